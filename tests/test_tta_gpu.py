"""Flip test-time augmentation at evaluation on the device: `mliis_view_gather` / `mliis_view_merge` (csrc/tta.hip, libmliis_tta.so) through
ops.view_gather / ops.view_merge, the `views=` keyword of the Learner's scoring methods, `Gecko(eval_views=...)` and `--eval-tta`.

The kernels copy words or round one sum and one product, so they are held to torch on the device bit for bit.  The learner is held, bit for
bit, to a restatement from twins that see the task mirrored on the host.  Orientation and averaging are checked independently of all that
against a float64 numpy reference that averages at FULL resolution (tests/tta_ref.py), pixels within tau of the decision excluded."""
import contextlib
import io
import json
import os
import random

import numpy as np
import pytest
import torch

import memcheck
import test_device_metrics_gpu as DM
import tta_ref as R
from test_save_predictions_gpu import _tree

pytestmark = pytest.mark.gpu

ALL_FLIPS = [(False, False), (False, True), (True, False), (True, True)]
SENT = 0x5A5A5A5A
BAND = 256       # sentinel words on either side of an output


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _banded(shape, d, shift=0):
    """(buffer, view): a float32 view of `shape` inside an int32 buffer of sentinels, `shift` words past a 16-byte boundary."""
    n = int(np.prod(shape))
    buf = torch.full((BAND + n + BAND + 4,), SENT, dtype=torch.int32, device=d)
    return buf, buf[BAND + shift:BAND + shift + n].view(torch.float32).view(shape)


def _bands_intact(buf, n, shift=0):
    return bool((buf[:BAND + shift] == SENT).all()) and bool((buf[BAND + shift + n:] == SENT).all())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ gather
# one word | odd sizes, W C = 21 (word path) | W C = 24, two images (row quads) | the real row: 672 words, 168 quads | C = 2, W C = 12
GATHER_SHAPES = [(1, 1, 1, 3), (3, 5, 7, 3), (2, 8, 8, 3), (2, 6, 224, 3), (2, 5, 6, 2)]


@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_view_gather_equals_torch_indexing_and_flip_bit_for_bit(shape):
    d = dev()
    from mliis_amd import ops
    N, H, W, C = shape
    S = N + 2
    g = torch.Generator().manual_seed(N * 1000 + W)
    # any 32-bit pattern: NaN payloads, infinities and denormals are copied like everything else
    pool_t = torch.randint(-2 ** 31, 2 ** 31 - 1, (S, H, W, C), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    perm = ([S - 1, 0] + [0] * N)[:N] if N > 1 else [S - 1]          # a permutation into the larger pool, image 0 twice
    idx = torch.tensor(perm, dtype=torch.int32, device=d)
    n = N * H * W * C
    memcheck.reset_guards()
    pool = memcheck.guarded_input(pool_t)
    snap = memcheck.snapshot(pool)
    for flips in ALL_FLIPS:
        for ix in (None, idx):
            src = pool[:N] if ix is None else pool
            want = (pool[:N] if ix is None else pool[ix.long()]).view(torch.int32).flip(R.flip_dims(flips)).view(torch.float32)
            for shift in (0, 1):                                       # 16-byte aligned | off by 4 bytes: the word path
                buf, out = _banded(shape, d, shift)
                assert out.data_ptr() % 16 == 4 * shift
                got = ops.view_gather(src, ix, flips, out=out)
                torch.cuda.synchronize()
                assert got is out and _same_bits(out, want), (shape, flips, ix is not None, shift)
                assert _bands_intact(buf, n, shift), (shape, flips, shift)
            assert _same_bits(ops.view_gather(src, ix, flips), want)   # out allocated by the wrapper
    # a source off by 4 bytes under an aligned destination: quads stored, words loaded
    sbuf = torch.zeros(S * H * W * C + 5, dtype=torch.float32, device=d)
    off = sbuf[1:1 + S * H * W * C].view(S, H, W, C)
    off.copy_(pool)
    for flips in ALL_FLIPS:
        want = off[idx.long()].view(torch.int32).flip(R.flip_dims(flips)).view(torch.float32)
        assert _same_bits(ops.view_gather(off, idx, flips), want), (shape, flips)
    # a view name in place of the pair
    assert _same_bits(ops.view_gather(pool, idx, "hflip"), pool[idx.long()].view(torch.int32).flip((2,)).view(torch.float32))
    snap.assert_unchanged()
    assert torch.equal(idx.cpu(), torch.tensor(perm, dtype=torch.int32))
    memcheck.assert_guards()


def test_view_gather_refusals():
    d = dev()
    from mliis_amd import ops
    from mliis_amd._lib import MliisError
    src = torch.zeros(3, 4, 4, 3, device=d)
    idx = torch.tensor([2, 0], dtype=torch.int32, device=d)
    for bad in (lambda: ops.view_gather(src, idx.long(), (0, 1)), lambda: ops.view_gather(src.cpu(), None, (0, 1)),
                lambda: ops.view_gather(src, idx, (0, 1), out=torch.zeros(3, 4, 4, 3, device=d)),
                lambda: ops.view_gather(src, idx, (0, 1), out=torch.zeros(2, 4, 4, 3, device=d, dtype=torch.float64)),
                lambda: ops.view_gather(src.transpose(1, 2), None, (0, 1)), lambda: ops.view_gather(torch.zeros(3, 4, 4, 5, device=d), None, (0, 1)),
                lambda: ops.view_gather(src, None, "rot90"), lambda: ops.view_gather(src, None, (0, 1), out=src)):
        with pytest.raises(MliisError):
            bad()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ merge
MERGE_SHAPES = [(1, 1, 1, 2), (3, 5, 7, 2), (2, 16, 16, 2), (2, 56, 56, 2)]      # word path twice (odd Wd) | row quads twice (even Wd)
SCALES = [1.0, 0.5, float(np.float32(1.0) / np.float32(3.0)), 0.25]


def _logits(shape, g):
    t = torch.randn(shape, generator=g) * 3.0
    flat = t.view(-1)
    special = [float("inf"), float("-inf"), float("nan"), -0.0, 0.0]
    k = torch.randperm(flat.numel(), generator=g)[:min(flat.numel(), 3 * len(special))]
    for i, p in enumerate(k.tolist()):
        flat[p] = special[i % len(special)]
    return t


def _nan_equal_bits(got, want):
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(torch.where(gn, torch.zeros_like(got), got).view(torch.int32),
                                               torch.where(wn, torch.zeros_like(want), want).view(torch.int32))


@pytest.mark.parametrize("shape", MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_view_merge_equals_torch_bit_for_bit(shape):
    d = dev()
    from mliis_amd import ops
    g = torch.Generator().manual_seed(shape[1] * 100 + shape[2])
    n = int(np.prod(shape))
    memcheck.reset_guards()
    a0, b0 = _logits(shape, g), _logits(shape, g)
    a, b = memcheck.guarded_input(a0), memcheck.guarded_input(b0)
    snap = memcheck.snapshot(a, b)
    for flips in ALL_FLIPS:
        fb = b.flip(R.flip_dims(flips)) if R.flip_dims(flips) else b
        for scale in SCALES:
            st = torch.tensor(scale, dtype=torch.float32, device=d)
            want = (a + fb) * st
            want_b = fb * st
            for shift in ((0, 1) if scale == 0.5 else (0,)):           # (the off-by-4-bytes output once per flip: the word path)
                buf, out = _banded(shape, d, shift)
                assert ops.view_merge(out, a, b, flips, scale) is out
                torch.cuda.synchronize()
                assert _nan_equal_bits(out, want), (shape, flips, scale, shift)
                assert _bands_intact(buf, n, shift)
                out.view(torch.int32).fill_(SENT)
                ops.view_merge(out, None, b, flips, scale)              # no addition
                torch.cuda.synchronize()
                assert _nan_equal_bits(out, want_b), (shape, flips, scale, shift)
                assert _bands_intact(buf, n, shift)
                out.copy_(a)
                ops.view_merge(out, out, b, flips, scale)               # in place
                torch.cuda.synchronize()
                assert _nan_equal_bits(out, want), (shape, flips, scale, shift)
                assert _bands_intact(buf, n, shift)
        # a = None at scale 1 hands b's words on as they are: -0.0 stays -0.0 (NaNs stay NaNs)
        buf, out = _banded(shape, d)
        ops.view_merge(out, None, b, flips, 1.0)
        torch.cuda.synchronize()
        assert _nan_equal_bits(out, fb) and bool((out.view(torch.int32) == -2 ** 31).any()) == bool((b.view(torch.int32) == -2 ** 31).any())
    snap.assert_unchanged()
    memcheck.assert_guards()


def test_view_merge_refusals():
    d = dev()
    from mliis_amd import ops
    from mliis_amd._lib import MliisError
    a, b = torch.zeros(2, 4, 4, 2, device=d), torch.ones(2, 4, 4, 2, device=d)
    out = torch.full((2, 4, 4, 2), 7.0, device=d)
    for bad in (lambda: ops.view_merge(b, a, b, (0, 1), 0.5), lambda: ops.view_merge(out, a, b, (0, 1), 0.0),
                lambda: ops.view_merge(out, a, b, (0, 1), -0.5), lambda: ops.view_merge(out, a, b, (0, 1), float("inf")),
                lambda: ops.view_merge(out, a, b, (0, 1), float("nan")), lambda: ops.view_merge(out, a, b[:1], (0, 1), 0.5),
                lambda: ops.view_merge(out, a[:, :, :3], b, (0, 1), 0.5), lambda: ops.view_merge(out, a, None, (0, 1), 0.5),
                lambda: ops.view_merge(out, a.double(), b, (0, 1), 0.5), lambda: ops.view_merge(out.cpu(), a.cpu(), b.cpu(), (0, 1), 0.5)):
        with pytest.raises(MliisError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((b == 1.0).all())


# ------------------------------------------------------------------------------------------------ orientation and averaging, float64
F64_CASES = [((3, 16, 16, 64, 64), 0), ((2, 7, 5, 23, 19), 0)]       # ((N, Hd, Wd, H, W), seed)


def _f64_inputs(shape, seed):
    N, Hd, Wd, H, W = shape
    rng = np.random.default_rng([seed, Hd, W])
    return {k: (rng.normal(0.0, 3.0, (N, Hd, Wd, 2))).astype(np.float32) for k in ("a",) + R.ORDER}


@pytest.mark.parametrize("views", [("hflip",), ("vflip",), ("hvflip",), R.ORDER], ids=lambda v: "+".join(v))
@pytest.mark.parametrize("case", F64_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_merged_mask_against_a_float64_average_at_full_resolution(case, views):
    shape, seed = case
    N, Hd, Wd, H, W = shape
    maps = _f64_inputs(shape, seed)
    a, bs = maps["a"], {v: maps[v] for v in views}
    tau = R.tau_of(a, *bs.values())
    d64 = R.margin_f64(a, bs, H, W)
    inside = np.abs(d64) < tau
    # the reference alone: the band is (nearly) empty for these seeds, and the fp32 restatement of the device arithmetic stays deep inside it
    assert inside.sum() <= 1e-3 * inside.size, (int(inside.sum()), inside.size)
    err = float(np.abs(R.margin_f32(a, bs, H, W).astype(np.float64) - d64).max())
    print("tta f64", shape, views, "tau = %.3g" % tau, "fp32 emulation error = %.3g (%.3f tau)" % (err, err / tau), "in band", int(inside.sum()))
    assert err <= tau / 4
    d = dev()
    from mliis_amd import ops
    from mliis_amd.metrics import unpack_mask
    ta = torch.tensor(a, device=d)
    if len(views) == 1:
        merged = ops.view_merge(torch.empty_like(ta), ta, torch.tensor(bs[views[0]], device=d), views[0], 0.5)
    else:      # the learner's sequence: the running sum of the mirrored views, then the in-place merge with the identity view
        acc = torch.empty_like(ta)
        for k, v in enumerate(views):
            ops.view_merge(acc, acc if k else None, torch.tensor(bs[v], device=d), v, 1.0)
        merged = ops.view_merge(ta, ta, acc, (False, False), 0.25)
    bits, _ = ops.mask_pack(merged, (H, W))
    torch.cuda.synchronize()
    mask = unpack_mask(bits.cpu().numpy(), H, W)
    wrong = (mask != (d64 > 0)) & ~inside
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:5].tolist())


# ------------------------------------------------------------------------------------------------ learner
H = 64
VIEW_SETS = [("hflip",), ("vflip",), ("hvflip",), ("hflip", "vflip"), ("hflip", "vflip", "hvflip")]
BATCHES = [[5, 6], [0, 1, 2, 3, 4, 6], [4, 6, 0, 2, 5, 1]]     # the transductive batch | the per-sample batch | a permutation of that size


def _learner():
    from mliis_amd.learner import Learner
    return Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=3, learning_rate=5e-3)


@pytest.fixture(scope="module")
def twins():
    """(A, B, C, x, y): three learners in the same trained-for-two-steps state; A scores with views, B sees the task mirrored on the host,
    C never scores."""
    dev()
    x, y = DM._task(7, H, 31)
    Ls = [_learner() for _ in range(3)]
    for L in Ls:
        L.load_task(x, y)
        for _ in range(2):
            L.inner_step([0, 1, 2, 3, 4])
        L.synchronize()
    yield Ls[0], Ls[1], Ls[2], x, y
    for L in Ls:
        L.close()


def _small(L, idx, training=False):
    L.score_resident(idx, training=training)
    return L._plan(len(idx), infer=True).small.clone()


def _expected(A, merged, idx):
    """What the existing kernels give on the merged logits: counts, masks, histogram, and the host path's mask."""
    from mliis_amd import ops
    from mliis_amd.metrics import unpack_mask
    ix = torch.tensor(idx, dtype=torch.int32, device=merged.device)
    counts = ops.mask_iou_counts(merged, A.shots_y, ix, (H, H)).cpu().numpy().astype(np.int64)
    bits, _ = ops.mask_pack(merged, (H, H))
    hist = ops.prob_histogram(merged, (H, H), A.shots_y, ix).cpu().numpy().astype(np.int64)
    logits = ops.resize_bilinear_fwd(merged, (H, H))
    _, _, pred = ops.softmax_ce(logits, torch.zeros_like(logits), None, want_grad=False, want_pred=True)
    torch.cuda.synchronize()
    return counts, unpack_mask(bits.cpu().numpy(), H, H), hist, (pred[..., 1] > 0.5).cpu().numpy()


def _merged(z_id, zs, views):
    """The stated formula in torch: s summed left to right in canonical order, the first term taken as it is."""
    s = None
    for v in R.ORDER:
        if v in views:
            t = zs[v].flip(R.flip_dims(R.FLIPS[v]))
            s = t if s is None else s + t
    return (z_id + s) * torch.tensor(np.float32(1.0 / (len(views) + 1)), device=z_id.device)


def test_learner_views_equal_the_restatement_from_mirrored_twins(twins):
    A, B, C, x, y = twins
    cases = [(tuple(b), False) for b in BATCHES] + [((5, 6), True)]      # (batch statistics last: such passes move the BN averages)
    # the mirrored twins' decoder-resolution logits: the whole task mirrored on the host, one load per view
    zs = {}
    for mode in (False, True):      # (B's batch-statistics passes move its BN averages too: all inference-mode passes come first)
        for v in R.ORDER:
            B.load_task(np.ascontiguousarray(R.flip_np(x, v)), np.ascontiguousarray(R.flip_np(y, v)))
            for idx, training in cases:
                if training == mode:
                    zs[(v, idx, training)] = _small(B, list(idx), training)
    before = A.export_all()
    theta0, bn0 = before["theta"].clone(), before["bn"].clone()
    for idx, training in cases:
        idx = list(idx)
        z_id = _small(A, idx, training)
        plain = A.score_resident(idx, training=training)
        for views in (VIEW_SETS if idx in BATCHES[:2] and not training else VIEW_SETS[::2]):
            merged = _merged(z_id, {v: zs[(v, tuple(idx), training)] for v in views}, views)
            counts, masks, hist, pmask = _expected(A, merged, idx)
            tag = (idx, training, views)
            assert np.array_equal(A.score_resident(idx, training=training, views=views), counts), tag
            assert torch.equal(A._plan(len(idx), infer=True).small, merged), tag
            m, c = A.mask_resident(idx, training=training, counts=True, views=views)
            assert np.array_equal(m, masks) and np.array_equal(c, counts), tag
            assert np.array_equal(A.mask_resident(idx, training=training, views=views), masks), tag
            m, c = A.mask_resident(idx, training=training, counts=True, last_only=True, views=views)
            assert np.array_equal(m, masks[-1:]) and np.array_equal(c, counts[-1:]), tag
            h, m = A.histogram_resident(idx, training=training, masks=True, views=views)
            assert np.array_equal(h, hist) and np.array_equal(m, masks), tag
            assert np.array_equal(A.histogram_resident(idx, training=training, last_only=True, views=views), hist[-1:]), tag
            pred = A.predict_resident(idx, training=training, views=views)
            assert np.array_equal((pred[..., 1] > 0.5).cpu().numpy(), pmask) and np.array_equal(pmask, masks), tag
            if not training and views == ("hflip", "vflip"):      # the order the views are asked in does not matter
                assert np.array_equal(A.score_resident(idx, views=("vflip", "hflip")), counts)
        if not training:
            print("tta learner", idx, "plain", plain[:, :2].tolist(), "all views", counts[:, :2].tolist())
            # views=() is the call without the keyword
            assert np.array_equal(A.score_resident(idx, views=()), plain)
            assert torch.equal(A._plan(len(idx), infer=True).small, z_id)
            # the training state: theta and the batch-norm tensors are those of before
            now = A.export_all()
            assert torch.equal(now["theta"], theta0) and torch.equal(now["bn"], bn0)
    A.synchronize()


def test_scoring_with_views_leaves_the_training_state_and_views_off_allocates_nothing(twins):
    A, B, C, x, y = twins
    from mliis_amd._lib import tta_lib
    L = _learner()                     # a fresh learner in the twins' state: no view was ever asked of it
    L.load_task(x, y)
    for _ in range(2):
        L.inner_step([0, 1, 2, 3, 4])
    idx = [5, 6]
    tta_lib.trace = calls = []
    try:
        rows = L.score_resident(idx)
        assert np.array_equal(L.score_resident(idx, views=()), rows)
        m0, h0 = L.mask_resident(idx, views=()), L.histogram_resident(idx, views=())
        p0 = L.predict_resident(idx, views=())
        assert calls == []
        for P in L.plans.values():
            assert P.view_x is None and P.view_acc is None
        assert np.array_equal(m0, L.mask_resident(idx)) and np.array_equal(h0, L.histogram_resident(idx))
        assert torch.equal(p0, L.predict_resident(idx))
        L.score_resident(idx, views=("hvflip", "hflip"))
        assert [n for n, _ in calls] == ["mliis_view_gather", "mliis_view_merge"] * 2 + ["mliis_view_merge"]
    finally:
        tta_lib.trace = None
    P = L._plan(2, infer=True)
    assert tuple(P.view_x.shape) == (2, H, H, 3) and tuple(P.view_acc.shape) == tuple(P.small.shape)
    L.mask_resident([0, 1, 2, 3, 4, 6], views=("vflip",))
    # the next step after scoring with views: the loss and parameters of the twin that never scored
    la, lc = L.inner_step([0, 1, 2, 3, 4]), C.inner_step([0, 1, 2, 3, 4])
    L.synchronize(), C.synchronize()
    assert torch.equal(la, lc)
    sa, sc = L.export_all(), C.export_all()
    assert torch.equal(sa["theta"], sc["theta"]) and torch.equal(sa["bn"], sc["bn"])
    for bad in (("rot90",), ("hflip", "hflip"), ("hflip", "vflip", "hflip")):
        for call in (L.score_resident, L.mask_resident, L.histogram_resident, L.predict_resident):
            with pytest.raises(ValueError):
                call(idx, views=bad)
    L.close()


# ------------------------------------------------------------------------------------------------ meta-learner
@pytest.mark.parametrize("transductive", [False, True])
def test_evaluate_with_views_returns_the_same_floats_on_all_four_paths(transductive, tmp_path):
    d = dev()
    from mliis_amd import metrics
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask
    from mliis_amd.predictions import PredictionWriter
    from mliis_amd.reptile import Gecko
    tasks = []
    for i in range(2):
        x, y = DM._task(9, H, 60 + i)
        tasks.append(DeviceTask("t%d" % i, torch.tensor(x).to(d), torch.tensor(y).to(d)))
    mk = lambda seed: Learner(image_size=H, seed=seed, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd")   # noqa: E731
    L = mk(2)
    lanes_cases = [()] if transductive else [(), (mk(77),)]
    theta0 = L.export_all()["theta"].clone()
    for lanes in lanes_cases:
        res = {}
        paths = {"host": {}, "device": {"device_metrics": True},
                 "writer": {"device_metrics": True, "prediction_writer": PredictionWriter(str(tmp_path / ("w%d" % len(lanes))))},
                 "host writer": {"prediction_writer": PredictionWriter(str(tmp_path / ("h%d" % len(lanes))))},
                 "sweep": {"device_metrics": True, "threshold_sweep": metrics.ThresholdSweep()}}
        for name, kw in paths.items():
            for views in ((), ("hflip",)):
                random.seed(11)
                np.random.seed(11)
                g = Gecko(L, rng_mode="reference", transductive=transductive, lanes=lanes, eval_views=views, **kw)
                with contextlib.redirect_stdout(io.StringIO()):
                    res[(name, views)] = g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=3, eval_all_tasks=True, test_shots=4)
                assert torch.equal(L.export_all()["theta"], theta0)          # the learner's state is restored
        for views in ((), ("hflip",)):
            for name in paths:
                assert res[(name, views)] == res[("host", views)], (name, views, lanes)
        print("tta evaluate", transductive, len(lanes), res[("host", ())][0], res[("host", ("hflip",))][0])
        assert _tree(str(tmp_path / ("w%d" % len(lanes)))) == _tree(str(tmp_path / ("h%d" % len(lanes))))      # (the last pass's masks: with views)
    for ln in [L] + list(lanes_cases[-1]):
        ln.close()


# ------------------------------------------------------------------------------------------------ command line
TTA = ["--eval-tta", "vflip", "hflip"]      # (given out of order: the run is that of hflip vflip)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    dev()
    d1 = str(tmp_path_factory.mktemp("tta") / "ckpt")
    DM._run(DM.BASE + ["--meta-iters", "1", "--eval-interval", "0", "--checkpoint", d1])
    return d1


def _pass(d1, extra):
    """(printed lines, meta-test_results.json's bytes, the sweep file or None) of one --pretrained run."""
    res, swp = os.path.join(d1, "meta-test_results.json"), os.path.join(d1, "meta-test_threshold_sweep.json")
    for f in (res, swp):
        if os.path.exists(f):
            os.remove(f)
    out = DM._run(DM.BASE + ["--pretrained", "--checkpoint", d1] + extra)
    assert "Meta-training..." not in out
    lines = [ln for ln in out.splitlines() if not ln.startswith("Experiment ")]
    return lines, open(res, "rb").read(), (json.load(open(swp)) if os.path.exists(swp) else None)


def _printed_mean(lines):
    return float(next(ln for ln in lines if ln.startswith("Mean IoU over all meta-test tasks: ")).split(": ")[1])


def test_cli_tta_writes_the_same_results_on_every_scoring_path(trained, tmp_path):
    host_lines, host_res, none = _pass(trained, TTA)
    assert none is None
    dm_lines, dm_res, _ = _pass(trained, ["--device-metrics"] + TTA)
    assert dm_res == host_res and _printed_mean(dm_lines) == _printed_mean(host_lines)
    lines, res, doc = _pass(trained, ["--device-metrics", "--threshold-sweep"] + TTA)
    assert res == host_res and lines == dm_lines
    assert doc["tta_views"] == ["hflip", "vflip"] and doc["iou_at_0.5"] == doc["mean_iou"][127] == _printed_mean(lines)
    roots = [str(tmp_path / "p0"), str(tmp_path / "p1")]
    a_lines, a_res, _ = _pass(trained, ["--save-predictions", roots[0]] + TTA)
    b_lines, b_res, _ = _pass(trained, ["--device-metrics", "--save-predictions", roots[1]] + TTA)
    assert a_res == b_res == host_res
    trees = [_tree(r) for r in roots]
    assert trees[0] == trees[1] and len(trees[0]) == 2 * 5          # the same PNG bytes: task evaluations x test shots
    print("tta cli mean IoU", _printed_mean(host_lines))


def test_cli_without_the_flag_is_the_run_it_always_was(trained):
    from mliis_amd._lib import tta_lib
    tta_lib.trace = calls = []
    try:
        lines, res, doc = _pass(trained, ["--device-metrics", "--threshold-sweep"])
        host_lines, host_res, _ = _pass(trained, [])
    finally:
        tta_lib.trace = None
    assert calls == [] and "tta_views" not in doc and res == host_res and _printed_mean(lines) == _printed_mean(host_lines)
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        DM._run(DM.BASE + ["--pretrained", "--checkpoint", trained, "--eval-tta", "rot90"])
    with pytest.raises(ValueError, match="more than once"):
        DM._run(DM.BASE + ["--pretrained", "--checkpoint", trained, "--eval-tta", "hflip", "hflip"])
