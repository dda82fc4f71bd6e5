"""Scoring on the device: `mliis_mask_iou_counts` (csrc/score.hip, libmliis_score.so) through ops.mask_iou_counts, Learner.score_resident, the
`device_metrics` option of the meta-learners and `--device-metrics` of the command line.

The counts are integers, so every comparison here is exact: against the mask the existing path writes (resize_bilinear_fwd ->
softmax_ce(want_pred=True), the mask predict() returns) and, independently of the device's own resize, against a float64 oracle up to
the pixels whose two logits are closer than the fp32 rounding of the bilinear sum."""
import contextlib
import ctypes as C
import io
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import memcheck

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 64), (2, 18, 72), (1, 25, 100), (5, 16, 16), (2, 56, 224), (1, 96, 384)]   # (N, Hd, H); (5,16,16): identity resize
LABEL_VALUES = [0.0, 1.0, 0.49, 0.5, 0.51, 1.5, -0.7]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _host_counts(pred1, lab1):
    """{|P & L|, |P | L|, |P|, |L|} as metrics.iou forms P and L: np.round(...).astype(bool) of the channel-1 planes."""
    p, l = np.round(pred1).astype(bool), np.round(lab1).astype(bool)
    return [int(np.count_nonzero(p & l)), int(np.count_nonzero(p | l)), int(np.count_nonzero(p)), int(np.count_nonzero(l))]


def _case(N, Hd, H, seed, d):
    g = torch.Generator().manual_seed(seed)
    small = torch.randn(N, Hd, Hd, 2, generator=g) * 2.0
    S = N + 2
    perm = torch.randperm(S, generator=g)[:N].tolist()
    if N > 1:
        perm[-1] = perm[0]                     # a repeat: two predictions scored against the same label image
    vals = torch.tensor(LABEL_VALUES)
    l1 = vals[torch.randint(0, len(LABEL_VALUES), (S, H, H), generator=g)]
    labels = torch.stack([1.0 - l1, l1], dim=-1)
    return small.to(d), labels.contiguous().to(d), torch.tensor(perm, dtype=torch.int32, device=d)


def _reference_counts(small, labels, idx, H):
    """The counts of the existing path: resize launch -> softmax_ce's prediction mask -> host, against np.round(label)."""
    from mliis_amd import ops
    logits = ops.resize_bilinear_fwd(small, (H, H))
    _, _, pred = ops.softmax_ce(logits, labels, idx, want_grad=False, want_pred=True)
    torch.cuda.synchronize()
    pred, lab, ix = pred.cpu().numpy(), labels.cpu().numpy(), idx.cpu().tolist()
    return [_host_counts(pred[n, ..., 1], lab[ix[n], ..., 1]) for n in range(len(ix))], pred, lab


@pytest.mark.parametrize("N,Hd,H", SHAPES)
def test_counts_equal_the_mask_of_the_existing_path(N, Hd, H):
    d = dev()
    from mliis_amd import metrics, ops
    small, labels, idx = _case(N, Hd, H, 7 * N + Hd, d)
    if (N, Hd, H) == (3, 16, 64):   # image 0: an empty mask against an empty label (0, 0.49 and 0.5 all round to 0: half to even)
        small[0, ..., 0], small[0, ..., 1] = 5.0, -5.0
        empty = torch.tensor([0.0, 0.49, 0.5], device=d)[torch.randint(0, 3, (H, H), device=d)]
        labels[idx[0].item(), ..., 1] = empty
        labels[idx[0].item(), ..., 0] = 1.0 - empty
    want, pred, lab = _reference_counts(small, labels, idx, H)
    got = ops.mask_iou_counts(small, labels, idx, (H, H))
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, 4)
    got = got.cpu().tolist()
    print("counts", (N, Hd, H), got)
    assert got == want
    ix = idx.cpu().tolist()
    for n in range(N):
        assert metrics.iou_from_counts(got[n][0], got[n][1]) == metrics.iou(pred[n], lab[ix[n]])
    if (N, Hd, H) == (3, 16, 64):
        assert got[0] == [0, 0, 0, 0] and metrics.iou_from_counts(got[0][0], got[0][1]) == 1.0
    # without the index vector: prediction n against label image n
    got0 = ops.mask_iou_counts(small, labels, None, (H, H)).cpu().tolist()
    want0 = [_host_counts(pred[n, ..., 1], lab[n, ..., 1]) for n in range(N)]
    assert got0 == want0


def test_near_ties_follow_the_threshold_rule():
    """z0 = 0 and z1 a few ulps of 1.0 either side of it, through the identity resize: the mask is softmax_ce's p1 > 0.5 (p = 0.5
    exactly leaves both channels 0), which is not the sign of z1 - z0."""
    d = dev()
    from mliis_amd import ops
    H = 16
    cyc = [0.0, 1e-8, -1e-8, 6e-8, -6e-8, 1.2e-7, -1.2e-7, 1e-6, -1e-6, 1.0, -1.0]
    z1 = torch.tensor([cyc[i % len(cyc)] for i in range(H * H)], dtype=torch.float32).reshape(1, H, H)
    small = torch.stack([torch.zeros_like(z1), z1], dim=-1).contiguous().to(d)
    g = torch.Generator().manual_seed(3)
    l1 = torch.randint(0, 2, (1, H, H), generator=g).float()
    labels = torch.stack([1.0 - l1, l1], dim=-1).contiguous().to(d)
    _, _, pred = ops.softmax_ce(small, labels, None, want_grad=False, want_pred=True)   # the identity resize: logits == small
    torch.cuda.synchronize()
    want = [_host_counts(pred.cpu().numpy()[0, ..., 1], labels.cpu().numpy()[0, ..., 1])]
    got = ops.mask_iou_counts(small, labels, None, (H, H)).cpu().tolist()
    print("near-tie counts", got, "pixels with z1 > z0:", int((z1 > 0).sum()))
    assert got == want
    assert _reference_counts(small, labels, torch.zeros(1, dtype=torch.int32, device=d), H)[0] == want


@pytest.mark.parametrize("N,Hd,H,exact", [(3, 16, 64, True), (2, 18, 72, True), (1, 25, 100, True), (2, 56, 224, True), (1, 96, 384, False)])
def test_counts_against_a_float64_resize(N, Hd, H, exact):
    """Independent of the device's resize: F.interpolate(align_corners=True) in float64, mask = z1 > z0.  A pixel is "in margin" when
    |z1 - z0| < 1e-5 there; an fp32 bilinear sum of |values| <= 5 carries ~2e-6 of rounding per channel, so outside the margin the
    device cannot disagree: every count may differ from the oracle's by at most the image's in-margin pixels.  For seed 0 the three small
    cases and 224 x 224 have none (they must match exactly), 384 x 384 has one; a torch build that draws differently fails the
    precondition below instead of hiding a case."""
    d = dev()
    from mliis_amd import ops
    small64 = torch.randn(N, 2, Hd, Hd, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    up = F.interpolate(small64, size=(H, H), mode="bilinear", align_corners=True)
    diff = up[:, 1] - up[:, 0]
    P = (diff > 0).numpy()
    in_margin = (diff.abs() < 1e-5).reshape(N, -1).sum(dim=1).tolist()
    print("in-margin pixels", (N, Hd, H), in_margin, "min |z1 - z0|", float(diff.abs().min()))
    assert sum(in_margin) <= 8
    if exact:
        assert sum(in_margin) == 0
    l1 = torch.randint(0, 2, (N, H, H), generator=torch.Generator().manual_seed(1)).float()
    labels = torch.stack([1.0 - l1, l1], dim=-1).contiguous().to(d)
    small = small64.permute(0, 2, 3, 1).float().contiguous().to(d)
    got = ops.mask_iou_counts(small, labels, None, (H, H)).cpu().tolist()
    Lb = l1.numpy().astype(bool)
    for n in range(N):
        want = [int((P[n] & Lb[n]).sum()), int((P[n] | Lb[n]).sum()), int(P[n].sum()), int(Lb[n].sum())]
        assert got[n][3] == want[3]
        assert all(abs(a - b) <= in_margin[n] for a, b in zip(got[n], want)), (n, got[n], want, in_margin[n])


def test_memory_contract():
    d = dev()
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, score_lib
    N, Hd, H = 3, 18, 72
    small_t, labels_t, idx = _case(N, Hd, H, 11, d)
    want, _, _ = _reference_counts(small_t, labels_t, idx, H)
    SENT = 0x5A5A5A5A
    memcheck.reset_guards()
    with memcheck.poisoned_allocations():
        small, labels = memcheck.guarded_input(small_t), memcheck.guarded_input(labels_t)
        buf = torch.full((N * 4 + 256,), SENT, dtype=torch.int32, device=d)
        counts = buf[:N * 4].view(N, 4)
        counts.fill_(0x7FFFFFFF)
        snap, idx0 = memcheck.snapshot(small, labels), idx.clone()
        score_lib.trace = calls = []
        try:
            out = ops.mask_iou_counts(small, labels, idx, (H, H), counts=counts)
        finally:
            score_lib.trace = None
        assert out is counts
        first = counts.cpu().tolist()
        ops.mask_iou_counts(small, labels, idx, (H, H), counts=counts)       # a second launch starts from zero again
        assert counts.cpu().tolist() == first == want
        assert ops.mask_iou_counts(small, labels, idx, (H, H)).cpu().tolist() == want     # counts allocated by the wrapper
        snap.assert_unchanged()
        assert torch.equal(idx, idx0)
        assert bool((buf[N * 4:] == SENT).all())
        memcheck.assert_guards()
    assert [name for name, _ in calls] == ["mliis_mask_iou_counts"]
    # the wrapper refuses operands the kernel would read as if they were packed, and a counts tensor of the wrong shape or type
    with pytest.raises(MliisError):
        ops.mask_iou_counts(small_t.transpose(1, 2), labels_t, idx, (H, H))
    wide = torch.zeros(N + 2, H, H, 3, device=d)
    with pytest.raises(MliisError):
        ops.mask_iou_counts(small_t, wide[..., :2], idx, (H, H))
    with pytest.raises(MliisError):
        ops.mask_iou_counts(small_t, labels_t, idx, (H, H), counts=torch.zeros(N, 3, dtype=torch.int32, device=d))
    with pytest.raises(MliisError):
        ops.mask_iou_counts(small_t, labels_t, idx, (H, H), counts=torch.zeros(N, 4, dtype=torch.float32, device=d))
    # an image smaller than the decoder's map: the library's error code and message, nothing launched
    tiny = torch.zeros(N + 2, 8, 8, 2, device=d)
    with pytest.raises(MliisError, match="smaller than the decoder"):
        ops.mask_iou_counts(small_t, tiny, idx, (8, 8))
    c = torch.zeros(N, 4, dtype=torch.int32, device=d)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw, last_error = score_lib.raw("mliis_mask_iou_counts"), score_lib.raw("mliis_score_last_error")
    assert raw(p(small_t), p(tiny), p(idx), N, Hd, Hd, 8, 8, p(c), st) == -1 and b"smaller" in last_error()
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Hd, H, Hd - 1, p(c), st) == -1
    assert raw(p(small_t), p(labels_t), p(idx), 0, Hd, Hd, H, H, p(c), st) == -1
    assert raw(p(small_t), p(labels_t), p(idx), N, 1, 1, 1, 1, p(c), st) == -1          # a 1 x 1 image: refused, as by the resize launch
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, 0, H, H, p(c), st) == -1
    assert raw(None, p(labels_t), p(idx), N, Hd, Hd, H, H, p(c), st) == -1 and b"null" in last_error()
    assert raw(p(small_t), None, p(idx), N, Hd, Hd, H, H, p(c), st) == -1
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Hd, H, H, None, st) == -1
    torch.cuda.synchronize()
    assert c.cpu().tolist() == [[0, 0, 0, 0]] * N


# ------------------------------------------------------------------------------------------------ learner
def _task(S, H, seed):
    from mliis_amd.metaseg import synthetic_task
    return synthetic_task(S, H, seed=seed)


def _predict_counts(L, idx, y, training=False):
    pred = L.predict_resident(idx, training=training).cpu().numpy()
    return np.asarray([_host_counts(pred[j, ..., 1], y[i, ..., 1]) for j, i in enumerate(idx)], dtype=np.int64)


def test_score_resident_equals_predict_resident_and_leaves_the_training_state():
    dev()
    from mliis_amd.learner import Learner
    H = 64
    x, y = _task(7, H, 31)
    A, B = (Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=3, learning_rate=5e-3) for _ in range(2))
    for L in (A, B):          # B: the twin that never scores
        L.load_task(x, y)
        for _ in range(2):
            L.inner_step([0, 1, 2, 3, 4])
    cases = [[5, 6], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 6], [4, 3, 2, 1, 0]]   # transductive shape, per-sample shape, the training plan's size
    got = [A.score_resident(idx) for idx in cases]
    for idx, g in zip(cases, got):
        assert isinstance(g, np.ndarray) and g.dtype == np.int64 and g.shape == (len(idx), 4)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    for idx, g in zip(cases, got):
        want = _predict_counts(A, idx, y)
        print("score_resident", idx, g.tolist())
        assert np.array_equal(g, want), (idx, g, want)
    assert np.array_equal(got[1][:5], got[2][:5])                   # inference mode: an image's score does not depend on its batch
    for bad in ([7], [-1], [0, 16], []):
        with pytest.raises(ValueError):
            A.score_resident(bad)
    la, lb = A.inner_step([0, 1, 2, 3, 4]), B.inner_step([0, 1, 2, 3, 4])      # the step after scoring: the same loss and parameters, bit for bit
    A.synchronize(), B.synchronize()
    assert torch.equal(la, lb)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    for idx in cases[:2]:         # batch statistics (training=True)
        assert np.array_equal(A.score_resident(idx, training=True), _predict_counts(A, idx, y, training=True))
    A.close(), B.close()


def test_score_resident_on_the_inference_plan_of_bf16_storage():
    dev()
    from mliis_amd.learner import Learner
    H = 64
    x, y = _task(7, H, 32)
    L = Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=4, learning_rate=5e-3, matmul_precision="bf16-storage")
    L.load_task(x, y)
    for _ in range(2):
        L.inner_step([0, 1, 2, 3, 4])
    for idx in ([5, 6], [0, 1, 2, 3, 4, 6], [4, 3, 2, 1, 0]):
        assert np.array_equal(L.score_resident(idx), _predict_counts(L, idx, y)), idx
    assert (5, "infer") in L.plans and L.plans[(5, "infer")].counts is not None and L.plans[5].counts is None
    L.inner_step([0, 1, 2, 3, 4])
    assert np.isfinite(L.loss_value())
    L.close()


# ------------------------------------------------------------------------------------------------ meta-learner
@pytest.mark.parametrize("transductive", [False, True])
def test_device_metrics_gives_the_same_ious_as_the_host_path(transductive):
    """Gecko.evaluate (and, per-sample, with a second learner as a lane) and _early_stopping_learn: device_metrics=True returns the very
    floats of device_metrics=False from the same state and seeds."""
    d = dev()
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask
    from mliis_amd.reptile import Gecko
    H = 64
    tasks = []
    for i in range(2):
        x, y = _task(9, H, 60 + i)
        tasks.append(DeviceTask("t%d" % i, torch.tensor(x).to(d), torch.tensor(y).to(d)))
    L = Learner(image_size=H, seed=2, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd")
    lanes_cases = [()] if transductive else [(), (Learner(image_size=H, seed=77, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd"),)]
    before = L.export_all()
    for lanes in lanes_cases:
        res = []
        for dm in (False, True):
            random.seed(11)
            np.random.seed(11)
            g = Gecko(L, rng_mode="reference", transductive=transductive, lanes=lanes, device_metrics=dm)
            with contextlib.redirect_stdout(io.StringIO()):
                res.append(g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=3, eval_all_tasks=True, test_shots=4))
        print("evaluate", transductive, len(lanes), res)
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and len(res[0][1]) == 2
    es = []
    L.load_task(tasks[0].images, tasks[0].labels)
    for dm in (False, True):
        random.seed(4)
        g = Gecko(L, rng_mode="reference", transductive=transductive, device_metrics=dm)
        with contextlib.redirect_stdout(io.StringIO()):
            es.append(g._early_stopping_learn([0, 1, 2, 3, 4], [5, 6, 7, 8], tasks[0].labels, 4, min_steps=1, max_steps=4, replacement=False,
                                              lr=5e-3, patience=2))
    print("early stopping", transductive, es)
    assert es[0] == es[1] and 1 <= es[0][0] <= 4
    after = L.export_all()
    assert torch.equal(before["theta"], after["theta"]) and torch.equal(before["bn"], after["bn"])
    for ln in [L] + list(lanes_cases[-1]):
        ln.close()


# ------------------------------------------------------------------------------------------------ command line
BASE = ["--image_size", "64", "--rsd", "2", "4", "--shots", "3", "--inner-batch", "4", "--inner-iters", "3", "--meta-batch", "2",
        "--eval-samples", "2", "--eval-iters", "2", "--eval-batch", "3", "--synthetic-tasks", "6", "--meta-step", "0.5",
        "--learning-rate", "0.005", "--skip-train-task-eval", "--sgd"]


def _run(argv):
    import run_metasegnet
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        run_metasegnet.main(argv)
    return buf.getvalue()


def test_cli_device_metrics_writes_the_same_results(tmp_path):
    dev()
    d1 = str(tmp_path / "a")
    _run(BASE + ["--meta-iters", "1", "--eval-interval", "0", "--checkpoint", d1])
    path = os.path.join(d1, "meta-test_results.json")
    outs = []
    for extra in ([], ["--device-metrics"]):
        os.remove(path)
        o = _run(BASE + ["--pretrained", "--checkpoint", d1] + extra)
        assert "Meta-training..." not in o and "Mean IoU over all meta-test tasks:" in o
        outs.append(open(path).read())
    assert outs[0] == outs[1] and len(json.loads(outs[0])) >= 1
