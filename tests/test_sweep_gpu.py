"""The evaluation threshold sweep on the device: `mliis_prob_histogram` (csrc/sweep.hip, libmliis_sweep.so) through ops.prob_histogram,
Learner.histogram_resident, the `threshold_sweep` sink of the meta-learners and `--threshold-sweep` / `--threshold-sweep-val` of the
command line.

A histogram is integers, so the comparisons against the tested scoring path are exact: the counts derived at k = 128 are those of
ops.mask_iou_counts bit for bit.  Independently of the device's own resize, every threshold k/256 is bracketed by a float64 numpy
reference evaluated at k/256 -/+ delta (no pixel excluded).

delta: the issue states 1e-5, with the fp32 evaluation of resize + softmax within 1.3e-6 of float64.  This module's fp32 numpy restatement
of the device arithmetic (_p1 with float32: fp32 source coordinates, weights, four fused multiply-adds, expf, reciprocal) observes, on
exactly the inputs below, max |p1_fp32 - p1_fp64| of
    (3, 5, 7, 19, 23):      6.4e-7 (N(0,3)), 2.3e-6 (N(0,8)), 2.6e-7 (engineered)
    (1, 8, 8, 8, 8):        6.2e-8, 5.9e-8, 2.1e-9
    (2, 56, 56, 224, 224):  1.14e-5 (N(0,3)), 2.87e-5 (N(0,8)), 1.25e-5 (engineered)
The 224 x 224 figures exceed delta / 4 = 2.5e-6: the fp32 source coordinate o * (Hd - 1) / (H - 1) is off by up to ~5e-6 of a decoder
pixel at coordinates near 55, and neighbouring logits of N(0, 8) differ by tens.  As the issue prescribes for that case, delta is widened
there to 8 x the value this emulation observes (DELTA_OF below: constants from the CPU emulation, never from the kernel); the widest,
2.3e-4, is still 17 times narrower than a bin (1/256 = 3.9e-3), so a bin that is off by one fails the bracket.  The other six cases keep
1e-5.  test_fp32_emulation_stays_within_the_deltas re-runs the emulation and holds it to delta / 8 (delta / 4 for the stated 1e-5)."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

import memcheck
import test_device_metrics_gpu as DM
from test_save_predictions_gpu import _tree

pytestmark = pytest.mark.gpu

# (N, Hd, Wd, H, W): upsampling, H W a multiple of neither the wave (64) nor the strip (4096), one partial workgroup, a permuting img_idx
# into 5 labels | the identity resize, one wave | the real shape: 13 strips per image (the last partial), a flush from 26 workgroups
SHAPES = [(3, 5, 7, 19, 23), (1, 8, 8, 8, 8), (2, 56, 56, 224, 224)]
DATA = ["n3", "n8", "engineered"]          # logits N(0, 3) | N(0, 8): saturated, bins 0 and 255 dominate | the engineered image
BINS = 256
# delta of check (c) per (shape, data): 1e-5 where the emulated fp32 error is below delta / 4, else 8 x the emulated error (module docstring)
DELTA_OF = {((2, 56, 56, 224, 224), "n3"): 8 * 1.2e-5, ((2, 56, 56, 224, 224), "n8"): 8 * 2.9e-5, ((2, 56, 56, 224, 224), "engineered"): 8 * 1.3e-5}


def _delta(shape, data):
    return DELTA_OF.get((tuple(shape), data), 1e-5)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ inputs and host references
_CASES = {}


def _inputs(shape, data):
    """(small [N,Hd,Wd,2], labels [S,H,W,2], idx [N]) as host float32 / int tensors; computed once per case and shared."""
    key = (tuple(shape), data)
    if key in _CASES:
        return _CASES[key]
    N, Hd, Wd, H, W = shape
    g = torch.Generator().manual_seed(1000 * DATA.index(data) + H)
    S = N + 2
    vals = torch.tensor(DM.LABEL_VALUES)
    l1 = vals[torch.randint(0, len(DM.LABEL_VALUES), (S, H, W), generator=g)]
    if data == "engineered":
        # along the decoder map's columns: z1 - z0 = +200 (p1 = 1 exactly) | +20 | at least two columns of equal logits (p1 = 0.5 exactly
        # wherever both source columns are equal ones: both channels see the same arithmetic) | -20 | -200 (p1 = 0 exactly in fp32).  The
        # sign changes over gentle slopes: a jump of 400 across one decoder pixel would turn the fp32 rounding of the source coordinate into
        # an error of p1 far above delta; on the steep parts p1 is within 2e-9 of 0 or 1
        base = torch.randn(N, Hd, Wd, generator=g) * 3.0
        n_eq = max(2, Wd // 4)
        c0 = (Wd - n_eq) // 2
        off = torch.zeros(Wd)
        off[:c0 - 1], off[c0 - 1] = 200.0, 20.0
        off[c0 + n_eq], off[c0 + n_eq + 1:] = -20.0, -200.0
        small = torch.stack([base, base + off[None, None, :]], dim=-1)
        l1[0] = 0.0                                   # an all-zero label
        l1[1] = 1.0                                   # an all-one label
        perm = [1, 0, 3][:N]                          # (N = 1: the all-one label through idx, the all-zero one without idx)
    else:
        small = torch.randn(N, Hd, Wd, 2, generator=g) * (3.0 if data == "n3" else 8.0)
        perm = torch.randperm(S, generator=g)[:N].tolist()
    labels = torch.stack([1.0 - l1, l1], dim=-1).contiguous()
    _CASES[key] = (small.contiguous(), labels, perm)
    return _CASES[key]


def _coord(O, I, dt):
    scale = dt(dt(I - 1) / dt(O - 1))
    f = (np.arange(O).astype(dt) * scale).astype(dt)
    i0 = np.minimum(np.floor(f).astype(np.int64), I - 1)
    return i0, np.minimum(i0 + 1, I - 1), (f - i0.astype(dt)).astype(dt)


def _p1(small, H, W, dt):
    """The channel-1 probability of every image pixel, [N,H,W] in dt: float64 = the reference; float32 = the restatement of the device
    arithmetic (src_coord, bilinear_weights, bilinear_sample's four fused multiply-adds in the order tl, tr, bl, br, softmax2)."""
    small = np.asarray(small, dtype=dt)
    N, Hd, Wd, _ = small.shape
    y0, y1, ly = _coord(H, Hd, dt)
    x0, x1, lx = _coord(W, Wd, dt)
    my, mx = (dt(1) - ly).astype(dt), (dt(1) - lx).astype(dt)
    weights = [(my[:, None] * mx[None, :]).astype(dt), (my[:, None] * lx[None, :]).astype(dt), (ly[:, None] * mx[None, :]).astype(dt),
               (ly[:, None] * lx[None, :]).astype(dt)]
    z = []
    for c in range(2):
        v = small[..., c]
        corners = [v[:, y0][:, :, x0], v[:, y0][:, :, x1], v[:, y1][:, :, x0], v[:, y1][:, :, x1]]
        o = np.zeros((N, H, W), dtype=dt)
        for w, t in zip(weights, corners):   # (a product of two fp32 values is exact in float64: one rounding of the sum, then to dt)
            o = (w[None].astype(np.float64) * t.astype(np.float64) + o.astype(np.float64)).astype(dt)
        z.append(o)
    m = np.maximum(z[0], z[1])
    e0, e1 = np.exp((z[0] - m).astype(dt)).astype(dt), np.exp((z[1] - m).astype(dt)).astype(dt)
    return (e1 * (dt(1) / (e0 + e1).astype(dt)).astype(dt)).astype(dt)


def _label_class(labels, perm):
    return np.rint(labels.numpy()[perm, ..., 1]) != 0       # (half to even; any non-zero value counts)


_REFS = {}


def _reference(shape, data):
    """Per image the ascending float64 p1 of all pixels and of the class-1 pixels, and the class-1 count (computed once per case)."""
    key = (tuple(shape), data)
    if key not in _REFS:
        small, labels, perm = _inputs(shape, data)
        p = _p1(small.numpy(), shape[3], shape[4], np.float64).reshape(shape[0], -1)
        L = _label_class(labels, perm).reshape(shape[0], -1)
        _REFS[key] = [(np.sort(p[n]), np.sort(p[n][L[n]]), int(L[n].sum())) for n in range(shape[0])]
    return _REFS[key]


def _above(sorted_p, t):
    """Number of entries > t, for an array of thresholds."""
    return len(sorted_p) - np.searchsorted(sorted_p, t, side="right")


def _device_hist(shape, data, d, with_idx=True, hist=None):
    from mliis_amd import ops
    small, labels, perm = _inputs(shape, data)
    idx = torch.tensor(perm, dtype=torch.int32, device=d) if with_idx else None
    out = ops.prob_histogram(small.to(d), shape[3:], labels.to(d), idx, hist=hist)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ the op
def test_fp32_emulation_stays_within_the_deltas():
    """The CPU check behind delta (needs no device): max |p1_fp32 - p1_fp64| of the module's own emulation on exactly the inputs below is
    at most delta / 8 for the widened cases and delta / 4 for the stated 1e-5."""
    for shape in SHAPES:
        for data in DATA:
            small = _inputs(shape, data)[0].numpy()
            err = float(np.abs(_p1(small, shape[3], shape[4], np.float32).astype(np.float64) - _p1(small, shape[3], shape[4], np.float64)).max())
            delta = _delta(shape, data)
            print("fp32 emulation", shape, data, "max |p1_fp32 - p1_fp64| = %.3g" % err, "delta = %.3g" % delta)
            assert err <= (delta / 4 if delta == 1e-5 else delta / 8 * 1.0000001), (shape, data, err, delta)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_histogram_against_the_scoring_kernel_and_a_float64_reference(shape, data):
    d = dev()
    from mliis_amd import metrics, ops
    N, Hd, Wd, H, W = shape
    small, labels, perm = _inputs(shape, data)
    hist = _device_hist(shape, data, d)
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (N, 2, BINS) and hist.is_cuda
    h = hist.cpu().numpy().astype(np.int64)
    assert h.min() >= 0
    counts = ops.mask_iou_counts(small.to(d), labels.to(d), torch.tensor(perm, dtype=torch.int32, device=d), (H, W)).cpu().numpy().astype(np.int64)
    derived = metrics.counts_from_histogram(h)
    print("hist", shape, data, "end bins", h[:, :, [0, 255]].reshape(N, -1).tolist(), "k=128", derived[:, 128].tolist())
    # (a) every pixel is counted once, and in its label's class
    assert h.sum(axis=(1, 2)).tolist() == [H * W] * N
    assert h[:, 1].sum(axis=1).tolist() == counts[:, 3].tolist()
    # (b) the counts at k = 128 are mask_iou_counts', bit for bit
    assert np.array_equal(derived[:, 128], counts), (derived[:, 128], counts)
    curve = metrics.iou_curve(h)
    assert [float(c) for c in curve[:, 128]] == [metrics.iou_from_counts(r[0], r[1]) for r in counts]
    # (c) every threshold k/256 bracketed by float64 at k/256 +/- delta; no pixel excluded
    delta = _delta(shape, data)
    ks = np.arange(1, BINS)
    for n, (p_all, p_fg, n_fg) in enumerate(_reference(shape, data)):
        assert n_fg == counts[n, 3]
        for got, ref in ((derived[n, 1:, 0], p_fg), (derived[n, 1:, 2], p_all)):
            lo, hi = _above(ref, ks / BINS + delta), _above(ref, ks / BINS - delta)
            bad = np.flatnonzero((got < lo) | (got > hi))
            assert bad.size == 0, (n, (bad[:5] + 1).tolist(), got[bad[:5]].tolist(), lo[bad[:5]].tolist(), hi[bad[:5]].tolist())
    if data == "engineered":
        # the exact probabilities sit where the rule puts them: p1 = 0.5 in bin 127 (not predicted), 1 in bin 255, 0 in bin 0
        p = _p1(small.numpy(), H, W, np.float64).reshape(N, -1)
        for n in range(N):
            assert h[n, :, 127].sum() >= int((p[n] == 0.5).sum()) > 0
            assert h[n, :, 255].sum() >= int((p[n] == 1.0).sum()) > 0 and h[n, :, 0].sum() >= int((p[n] < 1e-60).sum()) > 0   # (exp(-200) > 0 in float64)
        assert h[0, 0].sum() == 0 and (N == 1 or h[1, 1].sum() == 0)      # image 0 reads the all-one label (idx), image 1 the all-zero one
    # (d) the same bits again, and from a hist that held garbage (the zeroing launch)
    again = _device_hist(shape, data, d)
    assert torch.equal(again, hist)
    dirty = torch.full((N, 2, BINS), 0x7FFFFFF0, dtype=torch.int32, device=d)
    assert _device_hist(shape, data, d, hist=dirty) is dirty and torch.equal(dirty, hist)
    # without img_idx the labels are read in order
    plain = _device_hist(shape, data, d, with_idx=False).cpu().numpy().astype(np.int64)
    want = ops.mask_iou_counts(small.to(d), labels.to(d), None, (H, W)).cpu().numpy().astype(np.int64)
    assert np.array_equal(metrics.counts_from_histogram(plain)[:, 128], want)
    assert np.array_equal(plain.sum(axis=1), h.sum(axis=1))          # the probabilities do not depend on the labels


def test_memory_contract():
    d = dev()
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, sweep_lib
    shape = SHAPES[0]
    N, Hd, Wd, H, W = shape
    small_t, labels_t, perm = _inputs(shape, "n8")
    small_t, labels_t = small_t.to(d), labels_t.to(d)
    idx = torch.tensor(perm, dtype=torch.int32, device=d)
    want = _device_hist(shape, "n8", d).cpu().tolist()
    assert sweep_lib.size("mliis_prob_hist_bins") == BINS
    SENT = 0x5A5A5A5A
    words = N * 2 * BINS
    memcheck.reset_guards()
    with memcheck.poisoned_allocations():
        small, labels = memcheck.guarded_input(small_t), memcheck.guarded_input(labels_t)
        buf = torch.full((256 + words + 256,), SENT, dtype=torch.int32, device=d)
        hist = buf[256:256 + words].view(N, 2, BINS)
        hist.fill_(0x7FFFFFFF)
        snap, idx0 = memcheck.snapshot(small, labels), idx.clone()
        sweep_lib.trace = calls = []
        try:
            out = ops.prob_histogram(small, (H, W), labels, idx, hist=hist)
        finally:
            sweep_lib.trace = None
        assert out is hist and hist.cpu().tolist() == want
        assert ops.prob_histogram(small, (H, W), labels, idx).cpu().tolist() == want      # hist allocated by the wrapper
        snap.assert_unchanged()
        assert torch.equal(idx, idx0)
        assert bool((buf[:256] == SENT).all()) and bool((buf[256 + words:] == SENT).all())
        memcheck.assert_guards()
    assert [name for name, _ in calls] == ["mliis_prob_histogram"]
    # the wrapper refuses operands the kernel would read as if they were packed, and a hist of the wrong shape or type
    with pytest.raises(MliisError):
        ops.prob_histogram(small_t.transpose(1, 2), (H, W), labels_t, idx)
    with pytest.raises(MliisError):
        ops.prob_histogram(small_t, (H, W), torch.zeros(N + 2, H, W, 3, device=d)[..., :2], idx)
    with pytest.raises(MliisError):
        ops.prob_histogram(small_t, (H, W), labels_t, idx, hist=torch.zeros(N, 2, BINS - 1, dtype=torch.int32, device=d))
    with pytest.raises(MliisError):
        ops.prob_histogram(small_t, (H, W), labels_t, idx, hist=torch.zeros(N, 2, BINS, dtype=torch.float32, device=d))
    with pytest.raises(MliisError):
        ops.prob_histogram(small_t, (H, W), labels_t, idx[:2])
    tiny = torch.zeros(N + 2, 4, 4, 2, device=d)
    with pytest.raises(MliisError, match="smaller than the decoder"):
        ops.prob_histogram(small_t, (4, 4), tiny, idx)
    # the library's error codes; nothing is launched for any of them
    c = torch.full((N, 2, BINS), 7, dtype=torch.int32, device=d)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw, last_error = sweep_lib.raw("mliis_prob_histogram"), sweep_lib.raw("mliis_sweep_last_error")
    ARG, ALIGN = -1, -3
    assert raw(None, p(labels_t), p(idx), N, Hd, Wd, H, W, p(c), st) == ARG and b"null" in last_error()
    assert raw(p(small_t), None, p(idx), N, Hd, Wd, H, W, p(c), st) == ARG
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Wd, H, W, None, st) == ARG
    assert raw(p(small_t), p(tiny), p(idx), N, Hd, Wd, 4, 4, p(c), st) == ARG and b"smaller" in last_error()     # H < Hd
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Wd, H, Wd - 1, p(c), st) == ARG
    assert raw(p(small_t), p(labels_t), p(idx), 0, Hd, Wd, H, W, p(c), st) == ARG                                # N = 0
    assert raw(p(small_t), p(labels_t), p(idx), 65536, Hd, Wd, H, W, p(c), st) == ARG
    assert raw(p(small_t), p(labels_t), p(idx), N, 1, 1, 1, 1, p(c), st) == ARG
    assert raw(p(small_t, 4), p(labels_t), p(idx), N, Hd, Wd, H, W, p(c), st) == ALIGN and b"aligned" in last_error()
    assert raw(p(small_t), p(labels_t, 4), p(idx), N, Hd, Wd, H, W, p(c), st) == ALIGN
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Wd, H, W, p(c, 2), st) == ALIGN
    torch.cuda.synchronize()
    assert bool((c == 7).all())


# ------------------------------------------------------------------------------------------------ learner
def test_histogram_resident_equals_score_and_mask_resident():
    dev()
    from mliis_amd import metrics
    from mliis_amd.learner import Learner
    H = 64
    x, y = DM._task(7, H, 31)
    A, B = (Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=3, learning_rate=5e-3) for _ in range(2))
    for L in (A, B):          # B: the twin that never sweeps
        L.load_task(x, y)
        for _ in range(2):
            L.inner_step([0, 1, 2, 3, 4])
    for idx in ([5, 6], [0, 1, 2, 3, 4, 5], [4, 3, 2, 1, 0]):      # the transductive batch, the per-sample batch, the training plan's size
        rows, masks = A.score_resident(idx), A.mask_resident(idx)
        h = A.histogram_resident(idx)
        assert isinstance(h, np.ndarray) and h.dtype == np.int64 and h.shape == (len(idx), 2, BINS)
        assert np.array_equal(metrics.counts_from_histogram(h)[:, 128], rows), idx
        assert h.sum(axis=(1, 2)).tolist() == [H * H] * len(idx)
        last = A.histogram_resident(idx, last_only=True)
        assert last.shape == (1, 2, BINS) and np.array_equal(last[0], h[-1])
        h2, m2 = A.histogram_resident(idx, masks=True)
        assert np.array_equal(h2, h) and m2.dtype == bool and np.array_equal(m2, masks)
        h3, m3 = A.histogram_resident(idx, last_only=True, masks=True)
        assert np.array_equal(h3[0], h[-1]) and m3.shape == (1, H, H) and np.array_equal(m3[0], masks[-1])
        assert np.array_equal(A.mask_resident(idx, counts=True)[1], rows)      # the shared mask buffers still serve mask_resident
    P = A.plans[2]                       # (fp32 storage: training and inference share a plan per batch size)
    assert P.hist is not None and P.hist_pin.is_pinned() and tuple(P.hist_pin.shape) == (2, 2, BINS) and P.hist_pin is not P.counts_pin
    for bad in ([7], [-1], [0, 16], []):
        with pytest.raises(ValueError):
            A.histogram_resident(bad)
    la, lb = A.inner_step([0, 1, 2, 3, 4]), B.inner_step([0, 1, 2, 3, 4])      # the step after sweeping: the same loss and parameters
    A.synchronize(), B.synchronize()
    assert torch.equal(la, lb)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    # batch statistics (training=True; such a pass moves the batch-norm averages, as score_resident's does: after the twin comparison)
    assert np.array_equal(metrics.counts_from_histogram(A.histogram_resident([5, 6], training=True))[:, 128], A.score_resident([5, 6], training=True))
    A.close(), B.close()


@pytest.mark.parametrize("transductive", [False, True])
def test_the_sink_sees_every_task_and_the_ious_are_device_metrics(transductive):
    """Gecko.evaluate with a sink returns the very floats of device_metrics=True (sequentially and, per-sample, over a lane), and the sink
    receives every task's per-image curves, whose entry 128 is that image's IoU."""
    d = dev()
    import random
    from mliis_amd import metrics
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask
    from mliis_amd.reptile import Gecko
    H = 64
    tasks = []
    for i in range(2):
        x, y = DM._task(9, H, 60 + i)
        tasks.append(DeviceTask("t%d" % i, torch.tensor(x).to(d), torch.tensor(y).to(d)))
    L = Learner(image_size=H, seed=2, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd")
    lanes_cases = [()] if transductive else [(), (Learner(image_size=H, seed=77, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd"),)]
    for lanes in lanes_cases:
        res, sink = [], metrics.ThresholdSweep()
        for sweep in (None, sink):
            random.seed(11)
            np.random.seed(11)
            g = Gecko(L, rng_mode="reference", transductive=transductive, lanes=lanes, device_metrics=True, threshold_sweep=sweep)
            with contextlib.redirect_stdout(io.StringIO()):
                res.append(g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=3, eval_all_tasks=True, test_shots=4))
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and len(res[0][1]) == 2
        assert len(sink.passes) == 1 and sorted(n for n, _ in sink.passes[0]) == ["t0", "t1"]
        for name, curve in sink.passes[0]:
            assert float(curve[128]) == res[0][1][name]
        assert sink.summary()["iou_at_0.5"] == res[0][0] and int(sink.pooled.sum()) == 2 * 4 * H * H
    for ln in [L] + list(lanes_cases[-1]):
        ln.close()


# ------------------------------------------------------------------------------------------------ command line
VAL = ["--num_val_tasks", "2"]      # (with --pretrained the split leaves the test task where it was)


def _lines(out):
    return [ln for ln in out.splitlines() if not ln.startswith("Experiment ")]      # (the two lines that carry the clock)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    dev()
    d1 = str(tmp_path_factory.mktemp("sweep") / "ckpt")
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
    return _lines(out), open(res, "rb").read(), (json.load(open(swp)) if os.path.exists(swp) else None)


def _printed_mean(lines):
    return float(next(ln for ln in lines if ln.startswith("Mean IoU over all meta-test tasks: ")).split(": ")[1])


def _check_file(doc, lines, results):
    from mliis_amd import metrics
    assert doc["thresholds"] == [k / 256 for k in range(1, 256)] and len(doc["mean_iou"]) == 255
    assert doc["iou_at_0.5"] == doc["mean_iou"][127] == _printed_mean(lines)
    k = metrics.best_threshold_index([float("nan")] + doc["mean_iou"])
    assert doc["best_threshold"] == k / 256 and doc["iou_at_best"] == doc["mean_iou"][k - 1] >= doc["iou_at_0.5"]
    assert set(doc["tasks"]) == set(json.loads(results)) and all({"best_threshold", "iou_at_best"} <= set(v) for v in doc["tasks"].values())
    rel = doc["reliability"]
    assert len(rel["count"]) == 256 and sum(rel["count"]) == rel["pixels"] > 0 and 0.0 <= doc["ece"] == rel["ece"] <= 1.0


@pytest.mark.parametrize("extra", [[], ["--concurrent-tasks", "2"], ["--transductive"]], ids=["sequential", "lanes", "transductive"])
def test_cli_sweep_prints_and_writes_what_device_metrics_does(trained, extra):
    base_lines, base_res, none = _pass(trained, ["--device-metrics"] + extra)
    assert none is None                                               # without the flag no sweep file appears
    lines, res, doc = _pass(trained, ["--device-metrics", "--threshold-sweep"] + extra)
    assert lines == base_lines and res == base_res
    _check_file(doc, lines, res)
    print("sweep", extra, "iou@0.5", doc["iou_at_0.5"], "best", doc["best_threshold"], doc["iou_at_best"], "ece", doc["ece"])


def test_cli_sweep_saves_the_same_predictions(trained, tmp_path):
    roots = [str(tmp_path / "p0"), str(tmp_path / "p1")]
    base_lines, base_res, _ = _pass(trained, ["--device-metrics", "--save-predictions", roots[0]])
    lines, res, doc = _pass(trained, ["--device-metrics", "--threshold-sweep", "--save-predictions", roots[1]])
    assert [ln.replace(roots[1], roots[0]) for ln in lines] == base_lines and res == base_res
    _check_file(doc, lines, res)
    trees = [_tree(r) for r in roots]
    assert trees[0] == trees[1] and len(trees[0]) == 2 * 5          # the same PNG bytes: task evaluations x test shots


def test_cli_sweep_val_selects_on_the_validation_tasks(trained):
    from mliis_amd import metrics
    base_lines, base_res, _ = _pass(trained, ["--device-metrics"] + VAL)
    plain = _pass(trained, ["--device-metrics", "--threshold-sweep"] + VAL)[2]
    lines, res, doc = _pass(trained, ["--device-metrics", "--threshold-sweep-val"] + VAL)
    assert lines == base_lines and res == base_res                   # the val pass runs after the test pass and prints nothing
    _check_file(doc, lines, res)
    sel = doc.pop("selected_on_val")
    assert doc == plain                                              # the test half is that of --threshold-sweep alone
    k = metrics.best_threshold_index([float("nan")] + sel["val_mean_iou"])
    assert sel["threshold"] == k / 256 and sel["val_iou"] == sel["val_mean_iou"][k - 1]
    assert sel["test_iou_at_threshold"] == doc["mean_iou"][k - 1]
    with pytest.raises(ValueError, match="num_val_tasks"):
        DM._run(DM.BASE + ["--pretrained", "--checkpoint", trained, "--threshold-sweep-val"])
