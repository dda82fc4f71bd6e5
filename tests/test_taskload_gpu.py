"""Byte-resident tasks on the device: `mliis_task_expand_u8` (csrc/taskload.hip, libmliis_data.so) through ops.task_expand_u8,
Learner.load_task on the byte views of a metaseg.ByteTask, the meta-learners on ByteTasks and `--resident-dataset` /
`--stored-image-size` of the command line.

At the stored size everything is exact: the kernel's floats are tfrecord.parse_example's (metaseg.expand_bytes_host restates them), so
a learner, a meta-learner or the whole program fed bytes ends bit for bit where the one fed float arrays ends.  Resampled, the labels
are exact against the integer nearest rule and the image is held against the float64 restatement to 1.25e-4: per output value the fp32
chain rounds the two fractions (one division each), and each of the three a + (b - a) f steps a difference, a product and a sum (fused
or not) -- at most 8 roundings of values up to 255, 255 * 8 * 2^-24 = 1.22e-4."""
import contextlib
import io
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import memcheck

pytestmark = pytest.mark.gpu

H = 64
IMAGE_TOL = 1.25e-4
# (S, h, w, n, src_idx or None, byte offset of the pool inside its allocation)
SAME_SIZE = [
    (3, 7, 7, 3, None, 0),                       # row pitch 21 bytes, 147 pixels: nothing aligned, a short last group
    (2, 8, 12, 2, None, 0),                      # h w % 4 == 0, aligned pool: the word path
    (2, 8, 12, 2, None, 1),                      # the same shape from an odd address: the byte path
    (5, 10, 10, 9, [8, 8, 5, 2, 0], 0),          # a repeated, descending selection from a larger pool
    (3, 7, 7, 9, [6, 6, 1], 0),
    (2, 224, 224, 2, None, 0),                   # many workgroups, the word path at the size users run
]
RESAMPLED = [(3, (5, 7), (8, 12)), (3, (4, 4), (8, 8)), (3, (8, 8), (5, 5)), (3, (1, 3), (4, 6)), (1, (48, 48), (64, 64)),
             (1, (224, 224), (384, 384))]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _pool(n, h, w, seed, d, offset=0):
    """(images uint8 [n,h,w,3], masks uint8 [n,h,w]) on the host and on the device; the masks hold every byte value when they have room,
    the device copies start `offset` bytes into their allocations."""
    g = np.random.default_rng(seed)
    images = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    masks = g.integers(0, 256, (n, h, w), dtype=np.uint8)
    flat = masks.reshape(-1)
    k = min(256, flat.size)
    flat[:k] = g.permutation(256)[:k].astype(np.uint8)

    def up(a):
        buf = torch.zeros(a.size + offset, dtype=torch.uint8, device=d)
        buf[offset:] = torch.from_numpy(a.reshape(-1)).to(d)
        return buf[offset:].view(a.shape)
    return images, masks, up(images), up(masks)


def _idx(sel, d):
    return None if sel is None else torch.tensor(sel, dtype=torch.int32, device=d)


def _rows(sel, S):
    return list(range(S)) if sel is None else sel


@pytest.mark.parametrize("S,h,w,n,sel,offset", SAME_SIZE)
def test_same_size_is_bit_exact(S, h, w, n, sel, offset):
    d = dev()
    from mliis_amd import metaseg, ops
    images, masks, di, dm = _pool(n, h, w, 7 + S + h, d, offset)
    if masks.size >= 256:
        assert set(np.unique(masks)) == set(range(256))
    assert di.data_ptr() % 4 == offset % 4
    x = torch.full((S, h, w, 3), float("nan"), device=d)
    y = torch.full((S, h, w, 2), float("nan"), device=d)
    ops.task_expand_u8(di, dm, _idx(sel, d), x, y)
    torch.cuda.synchronize()
    rows = _rows(sel, S)
    x_ref, y_ref = metaseg.expand_bytes_host(images[rows], masks[rows], h, w)
    assert x.cpu().numpy().tobytes() == x_ref.tobytes()
    assert y.cpu().numpy().tobytes() == y_ref.tobytes()


def test_all_256_label_pairs_are_the_host_quotients():
    d = dev()
    from mliis_amd import ops
    m = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    x = torch.empty((1, 16, 16, 3), device=d)
    y = torch.empty((1, 16, 16, 2), device=d)
    ops.task_expand_u8(torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=d), torch.from_numpy(m).to(d), None, x, y)
    want = np.stack([255 - m, m], axis=-1).astype(np.float32) / 255.0
    assert y.cpu().numpy().tobytes() == want.tobytes() and not bool(x.any())


@pytest.mark.parametrize("S,src,dst", RESAMPLED)
def test_resampled_labels_exact_and_image_within_the_derived_bound(S, src, dst):
    d = dev()
    from mliis_amd import metaseg, ops
    (h, w), (Ho, Wo) = src, dst
    n = S + 1
    sel = None if S == 1 else [n - 1 - (k % 2) for k in range(S)]          # descending with a repeat
    images, masks, di, dm = _pool(n, h, w, 31 + h + Ho, d)
    x = torch.full((S, Ho, Wo, 3), float("nan"), device=d)
    y = torch.full((S, Ho, Wo, 2), float("nan"), device=d)
    ops.task_expand_u8(di, dm, _idx(sel, d), x, y)
    torch.cuda.synchronize()
    rows = _rows(sel, S)
    # labels: the integer nearest rule, then the byte's two quotients
    mi = [((2 * i + 1) * h) // (2 * Ho) for i in range(Ho)]
    mj = [((2 * j + 1) * w) // (2 * Wo) for j in range(Wo)]
    mm = masks[rows][:, mi][:, :, mj]
    y_want = np.stack([255 - mm, mm], axis=-1).astype(np.float32) / 255.0
    assert y.cpu().numpy().tobytes() == y_want.tobytes()
    x64, y64 = metaseg.expand_bytes_host(images[rows], masks[rows], Ho, Wo, dtype=np.float64)
    assert np.array_equal(y64, y_want.astype(np.float64))
    got = x.cpu().numpy()
    assert np.isfinite(got).all()
    err = float(np.abs(got.astype(np.float64) - x64).max())
    x32, _ = metaseg.expand_bytes_host(images[rows], masks[rows], Ho, Wo)
    print("resample {} -> {}: max |device - float64| = {:.3e}, max |numpy fp32 - float64| = {:.3e}".format(
        src, dst, err, float(np.abs(x32.astype(np.float64) - x64).max())))
    assert err <= IMAGE_TOL


@pytest.mark.parametrize("S,h,w,n,sel,offset", [c for c in SAME_SIZE if c[1] < 224] + [(3, 5, 7, 4, [3, 0, 3], 0)])
def test_memory_contract_every_element_written_guards_and_inputs_intact(S, h, w, n, sel, offset):
    d = dev()
    from mliis_amd import ops
    resample = (h, w) == (5, 7)
    Ho, Wo = (9, 11) if resample else (h, w)
    images, masks, di, dm = _pool(n, h, w, 3, d, offset)
    idx = _idx(sel, d)
    memcheck.reset_guards()
    with memcheck.poisoned_allocations():
        x = torch.empty((S + 1, Ho, Wo, 3), dtype=torch.float32, device=d)     # one image more than is written: it must stay poison
        y = torch.empty((S + 1, Ho, Wo, 2), dtype=torch.float32, device=d)
        assert bool(torch.isnan(x).all()) and bool(torch.isnan(y).all())
        keep = (di.clone(), dm.clone(), None if idx is None else idx.clone())
        ops.task_expand_u8(di, dm, idx, x[:S], y[:S])
    torch.cuda.synchronize()
    assert not bool(torch.isnan(x[:S]).any()) and not bool(torch.isnan(y[:S]).any())
    assert bool(torch.isnan(x[S:]).all()) and bool(torch.isnan(y[S:]).all())
    memcheck.assert_guards()
    assert torch.equal(di, keep[0]) and torch.equal(dm, keep[1]) and (idx is None or torch.equal(idx, keep[2]))
    assert np.array_equal(di.cpu().numpy(), images) and np.array_equal(dm.cpu().numpy(), masks)


def test_argument_errors_are_refused_before_any_launch():
    d = dev()
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, data_lib
    fn = data_lib.load().mliis_task_expand_u8
    last = data_lib.load().mliis_data_last_error
    S, n, h, w = 2, 3, 6, 5
    _, _, di, dm = _pool(n, h, w, 1, d)
    xb = torch.full((S * h * w * 3 + 4,), 7.0, device=d)
    yb = torch.full((S * h * w * 2 + 4,), 7.0, device=d)
    stream = torch.cuda.current_stream().cuda_stream
    good = dict(images=di.data_ptr(), masks=dm.data_ptr(), src_idx=None, S=S, n=n, h=h, w=w, H=h, W=w, x=xb.data_ptr(), y=yb.data_ptr())
    ERR_ARG, ERR_ALIGN = -1, -3
    cases = [("images", None, ERR_ARG), ("masks", None, ERR_ARG), ("x", None, ERR_ARG), ("y", None, ERR_ARG)]
    cases += [(k, v, ERR_ARG) for k in ("S", "n", "h", "w", "H", "W") for v in (0, -3)]
    cases += [("x", xb.data_ptr() + 4, ERR_ALIGN), ("y", yb.data_ptr() + 8, ERR_ALIGN)]
    for name, value, code in cases:
        a = dict(good)
        a[name] = value
        rc = fn(a["images"], a["masks"], a["src_idx"], a["S"], a["n"], a["h"], a["w"], a["H"], a["W"], a["x"], a["y"], stream)
        msg = last().decode()
        assert rc == code, (name, value, rc, msg)
        assert re.search(r"\b{}\b".format(name), msg), (name, msg)
    torch.cuda.synchronize()
    assert bool((xb == 7.0).all()) and bool((yb == 7.0).all())
    # ... and the wrapper's own checks: dtype, device, shapes, index vector
    x, y = xb[:S * h * w * 3].view(S, h, w, 3), yb[:S * h * w * 2].view(S, h, w, 2)
    bad = [lambda: ops.task_expand_u8(di.float(), dm, None, x, y), lambda: ops.task_expand_u8(di.cpu(), dm.cpu(), None, x, y),
           lambda: ops.task_expand_u8(di, dm[:, :-1].contiguous(), None, x, y), lambda: ops.task_expand_u8(di, dm, None, x, y[..., :1]),
           lambda: ops.task_expand_u8(di, dm, torch.zeros(S, dtype=torch.int64, device=d), x, y),
           lambda: ops.task_expand_u8(di, dm, torch.zeros(S + 1, dtype=torch.int32, device=d), x, y),
           lambda: ops.task_expand_u8(di[:1], dm[:1], None, x, y), lambda: ops.task_expand_u8(di, dm, None, x.double(), y)]
    for call in bad:
        with pytest.raises(MliisError):
            call()
    torch.cuda.synchronize()
    assert bool((xb == 7.0).all()) and bool((yb == 7.0).all())
    ops.task_expand_u8(di, dm, None, x, y)        # and the good call goes through
    torch.cuda.synchronize()
    assert not bool((x == 7.0).all()) and bool((xb[-4:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ Learner
def _task_pair(seed, shots, d, stored=H, size=H, name="t"):
    """The same task as a ByteTask on the device and as the float DeviceTask it expands to."""
    from mliis_amd.metaseg import ByteTask, DeviceTask, expand_bytes_host, synthetic_task_bytes
    xb, mb = synthetic_task_bytes(shots, stored, seed=seed)
    x, y = expand_bytes_host(xb, mb, size, size)
    return (ByteTask(name, torch.from_numpy(xb).to(d), torch.from_numpy(mb).to(d), size),
            DeviceTask(name, torch.from_numpy(x).to(d), torch.from_numpy(y).to(d)), (x, y))


@pytest.mark.parametrize("slots", [0, 8])
def test_learner_loads_byte_views_like_float_arrays(slots):
    d = dev()
    from mliis_amd.augment import Augmenter
    from mliis_amd.learner import Learner
    L = Learner(image_size=H, seed=3, use_graph=True, drop_connect=False, learning_rate=5e-3, augment_batch_capacity=slots)
    bt, _, (x, y) = _task_pair(5, 10, d)
    state = L.export_all()
    batches = [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 0, 1]]
    recipes = None
    if slots:
        aug = Augmenter(py=random.Random(4), npr=np.random.RandomState(4), verbose=False, fields=False)
        recipes = [[aug.plan((H, H, 3), 0.3) for _ in b] for b in batches]
        assert any(r is not None for rs in recipes for r in rs)

    def run(images, labels):
        L.import_all(state)
        with torch.cuda.stream(L.stream):
            L.shots_x.fill_(float("nan"))
            L.shots_y.fill_(float("nan"))
        L.load_task(images, labels)
        L.synchronize()
        S = L.n_shots
        assert L._aug_valid == 0
        shots = (L.shots_x[:S].cpu().clone(), L.shots_y[:S].cpu().clone())
        losses = []
        for j, b in enumerate(batches):
            idx = b
            if slots and not all(r is None for r in recipes[j]):
                idx = L.augment_batch(b, recipes[j])
            L.inner_step(idx)
            losses.append(L.loss_value())
        return S, shots, losses, L.export_all()["theta"].cpu().clone(), L._aug_valid
    a = run(x, y)
    vx, vy = bt.sample(10)
    b = run(vx, vy)
    assert a[0] == b[0] == 10 and a[4] == b[4]
    assert a[1][0].numpy().tobytes() == x.tobytes() and a[1][1].numpy().tobytes() == y.tobytes()
    assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
    assert a[2] == b[2] and all(np.isfinite(v) for v in a[2]), (a[2], b[2])
    assert torch.equal(a[3], b[3])
    # a selection that is not the pool's first S examples goes through the index vector; a pool on the host uploads its bytes
    L.load_task(vx[[7, 2, 2]], vy[[7, 2, 2]])
    L.synchronize()
    assert L.n_shots == 3 and L.shots_x[:3].cpu().numpy().tobytes() == x[[7, 2, 2]].tobytes()
    assert L.shots_y[:3].cpu().numpy().tobytes() == y[[7, 2, 2]].tobytes()
    from mliis_amd.metaseg import ByteTask
    hx, hy = ByteTask("host", bt.images_u8.cpu(), bt.masks_u8.cpu(), H).sample(4)
    L.load_task(hx, hy)
    L.synchronize()
    assert L.n_shots == 4 and L.shots_x[:4].cpu().numpy().tobytes() == x[:4].tobytes() and L.shots_y[:4].cpu().numpy().tobytes() == y[:4].tobytes()
    with pytest.raises(ValueError):
        L.load_task(vx, vy[:5])
    with pytest.raises(ValueError):
        L.load_task(*ByteTask("big", bt.images_u8, bt.masks_u8, H + 16).sample(2))
    with pytest.raises(ValueError):
        L.load_task(*ByteTask("many", bt.images_u8.repeat(2, 1, 1, 1), bt.masks_u8.repeat(2, 1, 1), H).sample(17))
    L.close()


def test_learner_resamples_a_task_stored_at_another_size():
    d = dev()
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import expand_bytes_host
    L = Learner(image_size=H, seed=3, use_graph=False, drop_connect=False)
    bt, _, _ = _task_pair(6, 6, d, stored=48, size=H)
    vx, vy = bt.sample(5)
    assert vx.shape == (5, H, H, 3) and bt.stored_size == (48, 48)
    L.load_task(vx, vy)
    L.synchronize()
    x64, y64 = expand_bytes_host(bt.images_u8[:5].cpu().numpy(), bt.masks_u8[:5].cpu().numpy(), H, H, dtype=np.float64)
    assert L.n_shots == 5 and np.array_equal(L.shots_y[:5].cpu().numpy().astype(np.float64), y64)
    assert float(np.abs(L.shots_x[:5].cpu().numpy().astype(np.float64) - x64).max()) <= IMAGE_TOL
    L.inner_step([0, 1, 2, 3])
    assert np.isfinite(L.loss_value())
    L.close()


# ------------------------------------------------------------------------------------------------ Gecko
def _reset_host_generators(seed):
    from mliis_amd import augment
    random.seed(seed)
    np.random.seed(seed)
    augment._SHARED_ORDER[:] = list(augment.PRISTINE_ORDER)


def _gecko_run(tasks, variant):
    """Two meta-iterations (meta-batch 2), then evaluate with host IoUs and with device metrics, all from fixed seeds."""
    from mliis_amd.learner import Learner
    from mliis_amd.reptile import Gecko
    mk = lambda seed, slots: Learner(image_size=H, seed=seed, use_graph=True, drop_connect=False, learning_rate=5e-3,   # noqa: E731
                                     augment_batch_capacity=slots)
    L = mk(1, 16 if variant == "augment" else 0)
    lanes = [mk(50, 0)] if variant == "lane" else []
    loads = []
    for ln in [L] + lanes:
        def load_task(images, labels, _load=ln.load_task):
            loads.append(type(images).__name__)
            return _load(images, labels)
        ln.load_task = load_task
    akw = dict(augment="device", aug_rate=0.7) if variant == "augment" else {}
    _reset_host_generators(13)
    with contextlib.redirect_stdout(io.StringIO()):
        meta = Gecko(L, rng_mode="per_task", seed=9, lanes=lanes, **akw)
        for _ in range(2):
            meta.train_step(list(tasks), num_shots=10, inner_batch_size=4, inner_iters=3, meta_step_size=0.5, meta_batch_size=2)
        assert meta._lanes_in_use() == (variant == "lane")
        st = L.export_all()
        theta, bn = st["theta"].cpu().clone(), st["bn"].cpu().clone()
        evals = []
        for dm in (False, True):
            _reset_host_generators(11)
            g = Gecko(L, rng_mode="reference", lanes=lanes, device_metrics=dm, **akw)
            evals.append(g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=2, eval_all_tasks=True))
    for ln in [L] + lanes:
        ln.close()
    return theta, bn, evals, loads


@pytest.mark.parametrize("variant", ["sequential", "lane", "augment"])
def test_gecko_on_byte_tasks_equals_gecko_on_float_tasks(variant):
    d = dev()
    pairs = [_task_pair(20 + i, 10, d, name="t%d" % i) for i in range(3)]
    a = _gecko_run([p[1] for p in pairs], variant)
    b = _gecko_run([p[0] for p in pairs], variant)
    assert set(a[3]) == {"Tensor"} and set(b[3]) == {"ByteView"} and len(a[3]) == len(b[3])      # every task went in as bytes
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert torch.equal(a[1], b[1]), float((a[1] - b[1]).abs().max())
    print("evaluate", variant, b[2])
    assert a[2] == b[2] and len(b[2][0][1]) == 3
    assert b[2][0] == b[2][1]                                                                      # host IoUs == device metrics
    assert all(0.0 <= v <= 1.0 for ev in b[2] for v in ev[1].values())


# ------------------------------------------------------------------------------------------------ the command line
def _run(argv):
    import run_metasegnet
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        run_metasegnet.main(argv)
    return buf.getvalue()


def _write_fss_shards(data_dir, size, n_tasks=6, examples=8, seed=0):
    from mliis_amd import tfrecord
    os.makedirs(data_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    names = tfrecord.fss_test_task_ids()[:2] + ["zz_train_task_%d" % i for i in range(n_tasks - 2)]
    for name in names:
        imgs = rng.integers(0, 256, size=(examples, size, size, 3), dtype=np.uint8)
        blocks = rng.random((examples, size // 8, size // 8)) < 0.3
        masks = (np.kron(blocks, np.ones((1, 8, 8))) * 255).astype(np.uint8)
        tfrecord.write_records(os.path.join(data_dir, name + ".tfrecord.gzip"), [tfrecord.make_example_bytes(i, m) for i, m in zip(imgs, masks)])
    return names


def _argv(data_dir, ckpt_dir, size=H):
    return ["--image_size", str(size), "--rsd", "2", "4", "--fss_1000", "--data-dir", data_dir, "--sgd", "--shots", "3", "--inner-batch", "4",
            "--inner-iters", "2", "--meta-batch", "2", "--meta-iters", "2", "--eval-interval", "0", "--eval-samples", "2", "--eval-iters", "2",
            "--eval-batch", "3", "--meta-step", "0.5", "--learning-rate", "0.005", "--skip-train-task-eval", "--checkpoint", ckpt_dir]


def test_main_with_a_resident_dataset_equals_main_without(tmp_path):
    dev()
    from mliis_amd import checkpoint as ckpt
    data_dir = str(tmp_path / "fss")
    names = _write_fss_shards(data_dir, H)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    out1 = _run(_argv(data_dir, d1))
    out2 = _run(_argv(data_dir, d2) + ["--resident-dataset"])
    for out in (out1, out2):
        assert "4 training tasks, 0 val tasks, 2 test tasks." in out and "Mean IoU over all meta-test tasks:" in out
    v1, v2 = ckpt.load(ckpt.latest_checkpoint(d1)), ckpt.load(ckpt.latest_checkpoint(d2))
    assert set(v1) == set(v2) and len(v1) > 10
    for k in v1:
        assert np.asarray(v1[k]).tobytes() == np.asarray(v2[k]).tobytes(), k
    r1, r2 = (json.load(open(os.path.join(dd, "meta-test_results.json"))) for dd in (d1, d2))
    assert r1 == r2 and sorted(r1) == sorted(n + ".tfrecord.gzip" for n in names[:2])


def test_main_resamples_shards_stored_at_another_size(tmp_path):
    dev()
    from mliis_amd import checkpoint as ckpt
    data_dir = str(tmp_path / "fss48")
    names = _write_fss_shards(data_dir, 48)
    d1 = str(tmp_path / "a")
    out = _run(_argv(data_dir, d1) + ["--stored-image-size", "48", "--resident-dataset"])
    assert "Mean IoU over all meta-test tasks:" in out
    vals = ckpt.load(ckpt.latest_checkpoint(d1))
    assert all(np.isfinite(v).all() for v in vals.values())
    res = json.load(open(os.path.join(d1, "meta-test_results.json")))
    assert sorted(res) == sorted(n + ".tfrecord.gzip" for n in names[:2])
    assert all(np.isfinite(float(x)) and 0.0 <= float(x) <= 1.0 for v in res.values() for x in v)
    with pytest.raises(ValueError, match="--resident-dataset"):
        _run(_argv(data_dir, str(tmp_path / "b")) + ["--stored-image-size", "48"])
    assert not os.path.exists(str(tmp_path / "b"))
