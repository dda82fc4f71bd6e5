"""Saving evaluation predictions on the device: `mliis_mask_pack` (csrc/score.hip, libmliis_score.so) through ops.mask_pack,
Learner.mask_resident, the `prediction_writer` option of the meta-learners and `--save-predictions` of the command line.

A mask is bits, so every comparison here is exact: against the mask the existing path writes (resize_bilinear_fwd ->
softmax_ce(want_pred=True)), against ops.mask_iou_counts, and -- independently of the device's own resize -- against a float64 oracle
whose in-margin pixels (|z1 - z0| < 1e-5) are asserted to be none at these shapes."""
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
import test_device_metrics_gpu as DM

pytestmark = pytest.mark.gpu

# (N, Hd, Wd, H, W): H*W a multiple of 256 | a multiple of 64 but not of 256 (the last workgroup: one live wave, three that must not
# store) | 16 valid bits in the last word | non-square, 19 valid bits | the identity resize
SHAPES = [(3, 16, 16, 64, 64), (2, 18, 18, 72, 72), (1, 25, 25, 100, 100), (2, 10, 7, 37, 23), (5, 16, 16, 16, 16)]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _case(N, Hd, Wd, H, W, seed, d):
    g = torch.Generator().manual_seed(seed)
    small = torch.randn(N, Hd, Wd, 2, generator=g) * 2.0
    S = N + 2
    perm = torch.randperm(S, generator=g)[:N].tolist()
    if N > 1:
        perm[-1] = perm[0]                     # a repeat: two predictions scored against the same label image
    vals = torch.tensor(DM.LABEL_VALUES)
    l1 = vals[torch.randint(0, len(DM.LABEL_VALUES), (S, H, W), generator=g)]
    labels = torch.stack([1.0 - l1, l1], dim=-1)
    return small.to(d), labels.contiguous().to(d), torch.tensor(perm, dtype=torch.int32, device=d)


def _existing_mask(small, H, W):
    """bool [N,H,W]: channel 1 of the prediction the existing path writes (resize launch -> softmax_ce's mask)."""
    from mliis_amd import ops
    logits = ops.resize_bilinear_fwd(small, (H, W))
    _, _, pred = ops.softmax_ce(logits, torch.zeros_like(logits), None, want_grad=False, want_pred=True)
    torch.cuda.synchronize()
    return pred[..., 1].cpu().numpy() > 0.5


def _popcounts(bits):
    return [sum(bin(int(w) & 0xFFFFFFFFFFFFFFFF).count("1") for w in row) for row in bits.cpu().tolist()]


def _check_against_the_existing_path(small, labels, idx, H, W):
    from mliis_amd import metrics, ops
    from mliis_amd._lib import score_lib
    N = small.shape[0]
    words = (H * W + 63) // 64
    assert score_lib.size("mliis_mask_pack_words", H, W) == words
    want = _existing_mask(small, H, W)
    bits, none = ops.mask_pack(small, (H, W))
    torch.cuda.synchronize()
    assert none is None and bits.dtype == torch.int64 and tuple(bits.shape) == (N, words) and bits.is_cuda
    got = metrics.unpack_mask(bits.cpu().numpy(), H, W)
    assert got.shape == want.shape and np.array_equal(got, want)
    pop = _popcounts(bits)
    assert pop == [int(want[n].sum()) for n in range(N)]                  # also: the tail bits of the last word are 0
    for ix in (idx, None):
        bits2, counts = ops.mask_pack(small, (H, W), labels, ix)
        ref = ops.mask_iou_counts(small, labels, ix, (H, W))
        torch.cuda.synchronize()
        assert counts.dtype == torch.int32 and tuple(counts.shape) == (N, 4)
        assert torch.equal(bits2, bits) and torch.equal(counts, ref)
        assert [row[2] for row in counts.cpu().tolist()] == pop
    return got, pop


@pytest.mark.parametrize("N,Hd,Wd,H,W", SHAPES)
def test_bits_equal_the_mask_of_the_existing_path(N, Hd, Wd, H, W):
    d = dev()
    small, labels, idx = _case(N, Hd, Wd, H, W, 7 * N + Hd, d)
    if N > 2:           # image 0 empty, image 1 full: all-zero and all-one words
        small[0, ..., 0], small[0, ..., 1] = 5.0, -5.0
        small[1, ..., 0], small[1, ..., 1] = -5.0, 5.0
    got, pop = _check_against_the_existing_path(small, labels, idx, H, W)
    print("mask_pack", (N, Hd, Wd, H, W), pop)
    if N > 2:
        assert pop[0] == 0 and pop[1] == H * W and not got[0].any() and got[1].all()


def test_near_ties_follow_the_threshold_rule():
    """The input of the counts kernel's near-tie test (z0 = 0, z1 a few ulps of 1.0 either side of it, identity resize): the bits are
    softmax_ce's p1 > 0.5, which is not the sign of z1 - z0."""
    d = dev()
    H = 16
    cyc = [0.0, 1e-8, -1e-8, 6e-8, -6e-8, 1.2e-7, -1.2e-7, 1e-6, -1e-6, 1.0, -1.0]
    z1 = torch.tensor([cyc[i % len(cyc)] for i in range(H * H)], dtype=torch.float32).reshape(1, H, H)
    small = torch.stack([torch.zeros_like(z1), z1], dim=-1).contiguous().to(d)
    l1 = torch.randint(0, 2, (1, H, H), generator=torch.Generator().manual_seed(3)).float()
    labels = torch.stack([1.0 - l1, l1], dim=-1).contiguous().to(d)
    got, pop = _check_against_the_existing_path(small, labels, torch.zeros(1, dtype=torch.int32, device=d), H, H)
    print("near-tie bits set", pop, "pixels with z1 > z0:", int((z1 > 0).sum()))


@pytest.mark.parametrize("N,Hd,Wd,H,W", SHAPES)
def test_bits_against_a_float64_resize(N, Hd, Wd, H, W):
    """Independent of the device's resize: F.interpolate(align_corners=True) in float64, mask = z1 > z0.  A pixel is "in margin" when
    |z1 - z0| < 1e-5 there (the existing counts test's margin: an fp32 bilinear sum of |values| <= 5 carries ~2e-6 of rounding per
    channel); the masks may differ at in-margin pixels only.  For seed 0 these five shapes have none (smallest gap 3.0e-5, at
    (2,18,18,72,72)), so the masks must be equal; a torch build that draws differently fails the precondition instead of hiding a case."""
    d = dev()
    from mliis_amd import metrics, ops
    small64 = torch.randn(N, 2, Hd, Wd, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    up = F.interpolate(small64, size=(H, W), mode="bilinear", align_corners=True)
    diff = up[:, 1] - up[:, 0]
    want = (diff > 0).numpy()
    in_margin = (diff.abs() < 1e-5).numpy()
    print("in-margin pixels", (N, Hd, Wd, H, W), int(in_margin.sum()), "min |z1 - z0|", float(diff.abs().min()))
    assert int(in_margin.sum()) == 0
    small = small64.permute(0, 2, 3, 1).float().contiguous().to(d)
    bits, _ = ops.mask_pack(small, (H, W))
    torch.cuda.synchronize()
    got = metrics.unpack_mask(bits.cpu().numpy(), H, W)
    assert not (got != want)[~in_margin].any()
    assert np.array_equal(got, want)


def test_memory_contract():
    d = dev()
    from mliis_amd import metrics, ops
    from mliis_amd._lib import MliisError, score_lib
    N, Hd, Wd, H, W = 2, 10, 7, 37, 23                  # 851 pixels: 14 words, 19 valid bits in the last; 4 workgroups, two waves of the last store nothing
    words, tail = 14, 19
    small_t, labels_t, idx = _case(N, Hd, Wd, H, W, 11, d)
    want = _existing_mask(small_t, H, W)
    want_counts = ops.mask_iou_counts(small_t, labels_t, idx, (H, W)).cpu().tolist()
    SENT, CSENT = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    memcheck.reset_guards()
    with memcheck.poisoned_allocations():
        small, labels = memcheck.guarded_input(small_t), memcheck.guarded_input(labels_t)
        buf = torch.full((N * words + 64,), SENT, dtype=torch.int64, device=d)
        bits = buf[:N * words].view(N, words)
        bits.fill_(-1)                                  # all ones: a word the launch skipped, or tail bits it left, would show
        cbuf = torch.full((N * 4 + 64,), CSENT, dtype=torch.int32, device=d)
        counts = cbuf[:N * 4].view(N, 4)
        snap, idx0 = memcheck.snapshot(small, labels), idx.clone()
        score_lib.trace = calls = []
        try:
            out, none = ops.mask_pack(small, (H, W), bits=bits)
        finally:
            score_lib.trace = None
        torch.cuda.synchronize()
        assert out is bits and none is None
        assert [name for name, _ in calls] == ["mliis_mask_pack"]
        assert calls[0][1][1] is None and calls[0][1][2] is None and calls[0][1][9] is None      # labels, idx, counts: null
        assert bool((cbuf == CSENT).all())                                                        # no counts work without labels
        first = bits.cpu().numpy().copy()
        assert np.array_equal(metrics.unpack_mask(first, H, W), want)
        assert all((int(first[n, -1]) & 0xFFFFFFFFFFFFFFFF) >> tail == 0 for n in range(N))       # the bits beyond H*W are written as 0
        assert bool((buf[N * words:] == SENT).all())                                              # nothing past N*words is touched
        bits.fill_(-1)
        score_lib.trace = calls = []
        try:
            out, cout = ops.mask_pack(small, (H, W), labels, idx, bits=bits, counts=counts)      # a second launch, with the counts
        finally:
            score_lib.trace = None
        torch.cuda.synchronize()
        assert out is bits and cout is counts and [name for name, _ in calls] == ["mliis_mask_pack"]
        assert np.array_equal(bits.cpu().numpy(), first) and counts.cpu().tolist() == want_counts
        ops.mask_pack(small, (H, W), labels, idx, bits=bits, counts=counts)                       # the counts start from zero again
        assert np.array_equal(bits.cpu().numpy(), first) and counts.cpu().tolist() == want_counts
        assert bool((buf[N * words:] == SENT).all()) and bool((cbuf[N * 4:] == CSENT).all())
        snap.assert_unchanged()
        assert torch.equal(idx, idx0)
        memcheck.assert_guards()
    # the wrapper refuses operands the kernel would read as if they were packed, and outputs of the wrong shape or type
    with pytest.raises(MliisError):
        ops.mask_pack(small_t.transpose(1, 2), (H, W))
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), bits=torch.zeros(N, words + 1, dtype=torch.int64, device=d))
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), bits=torch.zeros(N, words, dtype=torch.int32, device=d))
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), bits=torch.zeros(N, 2 * words, dtype=torch.int64, device=d)[:, ::2])
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), labels_t, idx, counts=torch.zeros(N, 3, dtype=torch.int32, device=d))
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), counts=torch.zeros(N, 4, dtype=torch.int32, device=d))    # counts without labels
    with pytest.raises(MliisError):
        ops.mask_pack(small_t, (H, W), torch.zeros(N + 2, H, W, 3, device=d)[..., :2], idx)
    with pytest.raises(MliisError, match="smaller than the decoder"):
        ops.mask_pack(small_t, (8, 6))
    # the library's own refusals: the documented codes, nothing launched
    b = torch.full((N * words + 1,), SENT, dtype=torch.int64, device=d)
    c = torch.full((N, 4), CSENT, dtype=torch.int32, device=d)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw, last_error = score_lib.raw("mliis_mask_pack"), score_lib.raw("mliis_score_last_error")
    ARG, ALIGN = -1, -3                                   # MLIIS_ERR_ARG, MLIIS_ERR_ALIGN (include/mliis_hip.h)
    assert raw(p(small_t, 4), None, None, N, Hd, Wd, H, W, p(b), None, st) == ALIGN and b"aligned" in last_error()
    assert raw(p(small_t), None, None, N, Hd, Wd, H, W, p(b, 4), None, st) == ALIGN                 # bits: 8-byte aligned
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Wd, H, W, p(b), p(c, 2), st) == ALIGN
    assert raw(p(small_t), None, None, N, Hd, Wd, H, W, None, None, st) == ARG and b"null" in last_error()
    assert raw(None, None, None, N, Hd, Wd, H, W, p(b), None, st) == ARG
    assert raw(p(small_t), p(labels_t), p(idx), N, Hd, Wd, H, W, p(b), None, st) == ARG and b"both or neither" in last_error()
    assert raw(p(small_t), None, p(idx), N, Hd, Wd, H, W, p(b), p(c), st) == ARG
    assert raw(p(small_t), None, None, N, Hd, Wd, 8, 6, p(b), None, st) == ARG and b"smaller" in last_error()
    assert raw(p(small_t), None, None, 0, Hd, Wd, H, W, p(b), None, st) == ARG
    assert raw(p(small_t), None, None, 65536, Hd, Wd, H, W, p(b), None, st) == ARG
    assert raw(p(small_t), None, None, N, 1, 1, 1, 1, p(b), None, st) == ARG                        # a 1 x 1 image, as the resize launch
    assert raw(p(small_t), None, None, N, Hd, 0, H, W, p(b), None, st) == ARG
    assert score_lib.size("mliis_mask_pack_words", 0, 5) <= 0 and score_lib.size("mliis_mask_pack_words", 5, -1) <= 0
    assert score_lib.size("mliis_mask_pack_words", 8, 8) == 1 and score_lib.size("mliis_mask_pack_words", 224, 224) == 784
    torch.cuda.synchronize()
    assert bool((b == SENT).all()) and bool((c == CSENT).all())


# ------------------------------------------------------------------------------------------------ learner
CASES = [[5, 6], [0, 1, 2, 3, 4, 5], [4, 3, 2, 1, 0]]   # transductive shape, per-sample shape, the training plan's size


def _centre(x, L, *others):
    """Shift the final layer's channel-1 bias (of L and, to the same value, of `others`) by the median of z1 - z0 over images x, so that
    about half of the pixels are foreground: a freshly initialised network predicts one class everywhere, which would test nothing."""
    _, lg = L.predict(torch.as_tensor(x), return_logits=True)
    shift = float((lg[..., 1] - lg[..., 0]).median())
    name = L.final_layer_scope + "/bias"
    bias = L.named_numpy()[name].copy()
    bias[1] -= shift
    for ln in (L,) + others:
        assert ln.load_named({name: bias}, strict=False) == 1


def _check_mask_resident(L, idx, training=False):
    want = L.predict_resident(idx, training=training)[..., 1].cpu().numpy() > 0.5
    rows = L.score_resident(idx, training=training)
    m = L.mask_resident(idx, training=training)
    assert isinstance(m, np.ndarray) and m.dtype == np.bool_ and m.shape == want.shape and np.array_equal(m, want), idx
    m2, c = L.mask_resident(idx, training=training, counts=True)
    assert np.array_equal(m2, want) and c.dtype == np.int64 and c.shape == (len(idx), 4) and np.array_equal(c, rows), idx
    assert [int(x.sum()) for x in m2] == c[:, 2].tolist()
    last = L.mask_resident(idx, training=training, last_only=True)
    assert last.shape == (1,) + want.shape[1:] and np.array_equal(last[0], want[-1])
    last, cl = L.mask_resident(idx, training=training, counts=True, last_only=True)
    assert np.array_equal(last[0], want[-1]) and cl.shape == (1, 4) and np.array_equal(cl[0], rows[-1])
    return m


def test_mask_resident_equals_predict_resident_and_leaves_the_training_state():
    dev()
    from mliis_amd.learner import Learner
    H = 64
    x, y = DM._task(7, H, 31)
    A, B = (Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=3, learning_rate=5e-3) for _ in range(2))
    for L in (A, B):          # B: the twin that never calls it
        L.load_task(x, y)
        for _ in range(2):
            L.inner_step([0, 1, 2, 3, 4])
    for idx in CASES:
        A.mask_resident(idx)
    A.mask_resident(CASES[1], counts=True, last_only=True)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    la, lb = A.inner_step([0, 1, 2, 3, 4]), B.inner_step([0, 1, 2, 3, 4])      # the step after it: the same loss and parameters, bit for bit
    A.synchronize(), B.synchronize()
    assert torch.equal(la, lb)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    for bad in ([7], [-1], [0, 16], []):
        with pytest.raises(ValueError):
            A.mask_resident(bad)
    _centre(x, A, B)          # (the same bias into both: the twins stay twins)
    sums = []
    for idx in CASES:
        m = _check_mask_resident(A, idx)
        print("mask_resident", idx, [int(v.sum()) for v in m])
        sums += [int(v.sum()) for v in m]
    assert any(0 < v < H * H for v in sums)                                   # (the masks are not all empty or all full)
    assert A.plans[2].bits is not None and A.plans[2].bits_pin.is_pinned()
    la, lb = A.inner_step([0, 1, 2, 3, 4]), B.inner_step([0, 1, 2, 3, 4])      # (replayed graphs by now)
    A.synchronize(), B.synchronize()
    assert torch.equal(la, lb)
    sa, sb = A.export_all(), B.export_all()
    assert torch.equal(sa["theta"], sb["theta"]) and torch.equal(sa["bn"], sb["bn"])
    for idx in CASES[:2]:         # batch statistics (training=True), last: as in predict(), such a pass moves the BN averages
        _check_mask_resident(A, idx, training=True)
    A.close(), B.close()


def test_mask_resident_on_the_inference_plan_of_bf16_storage():
    dev()
    from mliis_amd.learner import Learner
    H = 64
    x, y = DM._task(7, H, 32)
    L = Learner(image_size=H, rsd=[2, 4], optimizer="sgd", seed=4, learning_rate=5e-3, matmul_precision="bf16-storage")
    L.load_task(x, y)
    for _ in range(2):
        L.inner_step([0, 1, 2, 3, 4])
    _centre(x, L)
    for idx in CASES:
        _check_mask_resident(L, idx)
    assert (5, "infer") in L.plans and L.plans[(5, "infer")].bits is not None and L.plans[5].bits is None
    L.inner_step([0, 1, 2, 3, 4])
    assert np.isfinite(L.loss_value())
    L.close()


# ------------------------------------------------------------------------------------------------ meta-learner
def _tree(root):
    out = {}
    for dpath, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(dpath, f), root)] = open(os.path.join(dpath, f), "rb").read()
    return out


@pytest.mark.parametrize("transductive", [False, True])
def test_evaluate_with_a_writer_saves_the_same_masks_on_both_paths(tmp_path, monkeypatch, transductive):
    """Gecko.evaluate on one lane and on two: device_metrics False / True with a writer and without return the very same floats, the two
    paths write the same PNG files, and every saved mask scores the task's IoU against the label."""
    d = dev()
    from mliis_amd import metrics
    from mliis_amd import metaseg
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask
    from mliis_amd.predictions import PredictionWriter, overlay, read_png
    from mliis_amd.reptile import Gecko
    H, S, TEST = 64, 9, 4
    tasks, host = [], {}
    for i in range(2):
        x, y = DM._task(S, H, 60 + i)
        tasks.append(DeviceTask("t%d" % i, torch.tensor(x).to(d), torch.tensor(y).to(d)))
        host["t%d" % i] = (x, y)
    kw = dict(image_size=H, use_graph=True, drop_connect=False, learning_rate=5e-3, optimizer="sgd")
    L = Learner(seed=2, **kw)
    lane = Learner(seed=77, **kw)
    _centre(host["t0"][0], L)
    before = L.export_all()
    splits, split_indices = [], metaseg.split_indices

    def recording_split(*a, **k):                                        # the test images the evaluation drew, task by task
        out = split_indices(*a, **k)
        splits.append(out[1])
        return out

    monkeypatch.setattr(metaseg, "split_indices", recording_split)
    for lanes in ((), (lane,)):
        res, trees = {}, {}
        for dm in (False, True):
            for save in (True, False):
                random.seed(11)
                np.random.seed(11)
                root = str(tmp_path / "l{}_dm{}_s{}".format(len(lanes), int(dm), int(save)))
                writer = PredictionWriter(root, overlays=True) if save else None
                del splits[:]
                g = Gecko(L, rng_mode="reference", transductive=transductive, lanes=lanes, device_metrics=dm, prediction_writer=writer)
                with contextlib.redirect_stdout(io.StringIO()):
                    res[dm, save] = g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=3, eval_all_tasks=True,
                                               test_shots=TEST, eval_sample_num=1)
                trees[dm, save] = _tree(root)
                assert len(splits) == 2
        print("evaluate", transductive, len(lanes), res[True, True])
        assert res[False, False] == res[False, True] == res[True, False] == res[True, True] and len(res[True, True][1]) == 2
        assert trees[False, False] == trees[True, False] == {}
        assert trees[False, True] == trees[True, True]                    # the two paths: identical file for file
        assert sorted(trees[True, True]) == sorted(os.path.join("t%d" % i, "sample1_query%d_%s.png" % (j, kind))
                                                   for i in range(2) for j in range(TEST) for kind in ("mask", "overlay"))
        # each saved mask against its label gives the task's IoU (eval_all_tasks: the tasks in the order given; every run draws the same
        # splits from the same seed, so the last run's record serves)
        for task, test_idx in zip(tasks, splits):
            x, y = host[task.name]
            ious = []
            for j, t in enumerate(test_idx):
                stem = os.path.join(str(tmp_path / "l{}_dm1_s1".format(len(lanes))), task.name, "sample1_query%d" % j)
                m = read_png(stem + "_mask.png")
                ious.append(metrics.iou(np.stack([~m, m], axis=-1).astype(np.float32), y[t]))
                assert np.array_equal(read_png(stem + "_overlay.png"), overlay(x[t], m))
            assert float(np.nanmean(ious)) == res[True, True][1][task.name]
    after = L.export_all()
    assert torch.equal(before["theta"], after["theta"]) and torch.equal(before["bn"], after["bn"])
    L.close(), lane.close()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_saves_the_same_predictions_with_and_without_device_metrics(tmp_path):
    dev()
    d1 = str(tmp_path / "a")
    DM._run(DM.BASE + ["--meta-iters", "1", "--eval-interval", "0", "--checkpoint", d1])
    path = os.path.join(d1, "meta-test_results.json")
    outs, trees = [], []
    for k, extra in enumerate(([], ["--device-metrics"], ["--device-metrics", "--save-prediction-overlays"])):
        os.remove(path)
        root = str(tmp_path / ("p%d" % k))
        o = DM._run(DM.BASE + ["--pretrained", "--checkpoint", d1, "--save-predictions", root] + extra)
        assert "Meta-training..." not in o and "Mean IoU over all meta-test tasks:" in o
        outs.append(open(path).read())
        trees.append(_tree(root))
    os.remove(path)
    DM._run(DM.BASE + ["--pretrained", "--checkpoint", d1])
    assert outs[0] == outs[1] == outs[2] == open(path).read()            # saving changes no result
    results = json.loads(outs[0])
    passes = sum(len(v) for v in results.values())                       # task evaluations: one sampled task per pass x --eval-samples
    assert passes == 2
    assert trees[0] == trees[1] and len(trees[0]) == passes * 5          # tasks x eval samples x test shots (5)
    assert all(name.endswith("_mask.png") for name in trees[0])
    assert len(trees[2]) == 2 * len(trees[0]) and {k: v for k, v in trees[2].items() if k.endswith("_mask.png")} == trees[0]
