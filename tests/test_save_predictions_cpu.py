"""Host half of saving evaluation predictions (no GPU): the PNG writer / reader of mliis_amd.predictions, metrics.unpack_mask, overlay(),
Gecko._evaluate with a writer driven by a stub learner (mask_resident hands out prepared masks and counts), and the two flags with the
SAVE_PREDICTIONS switch."""
import contextlib
import io
import os
import random
import struct
import zlib

import numpy as np
import pytest

from mliis_amd import args as A
from mliis_amd import metrics
from mliis_amd import predictions as PR
from mliis_amd.reptile import FOMLIS, Gecko, SingleRank


# ------------------------------------------------------------------------------------------------ PNG
def _walk_chunks(data):
    """[(type, payload)], every CRC verified here (not through the module under test)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, pos = [], 8
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, payload = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + payload) & 0xFFFFFFFF, kind
        out.append((kind, payload))
        pos += 12 + n
    assert pos == len(data)
    return out


@pytest.mark.parametrize("W", [8, 23, 64, 100])
def test_png_round_trip_of_a_mask(tmp_path, W):
    rng = np.random.default_rng(W)
    H = 13
    mask = rng.random((H, W)) < 0.4
    mask[0, 0], mask[-1, -1], mask[0, -1] = True, True, False
    path = str(tmp_path / "m.png")
    PR.write_png(path, mask)
    chunks = _walk_chunks(open(path, "rb").read())
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 1, 0, 0, 0, 0)
    raw = zlib.decompress(chunks[1][1])
    stride = (W + 7) // 8
    assert len(raw) == H * (stride + 1) and all(raw[r * (stride + 1)] == 0 for r in range(H))          # filter type 0 on every row
    assert raw[1] >> 7 == 1                                                                            # pixel (0,0): the most significant bit
    got = PR.read_png(path)
    assert got.dtype == np.bool_ and got.shape == (H, W) and np.array_equal(got, mask)


def test_png_round_trip_of_an_rgb_image(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 23, 3), dtype=np.uint8)
    path = str(tmp_path / "c.png")
    PR.write_png(path, img)
    chunks = _walk_chunks(open(path, "rb").read())
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (23, 9, 8, 2, 0, 0, 0)
    got = PR.read_png(path)
    assert got.dtype == np.uint8 and np.array_equal(got, img)
    with pytest.raises(ValueError):
        PR.write_png(path, img.astype(np.float32))
    with pytest.raises(ValueError):
        PR.write_png(path, np.zeros((4, 4), np.uint8))
    # a damaged file is refused by the reader
    data = bytearray(open(path, "rb").read())
    data[-20] ^= 1
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError):
        PR.read_png(path)


def test_pillow_reads_the_same_pixels(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(1)
    path = str(tmp_path / "p.png")
    for W in (8, 23, 64, 100):
        mask = rng.random((11, W)) < 0.5
        PR.write_png(path, mask)
        with Image.open(path) as im:
            assert im.size == (W, 11) and im.mode == "1"
            assert np.array_equal(np.asarray(im.convert("L")) > 127, mask)                             # foreground white
    img = rng.integers(0, 256, (9, 23, 3), dtype=np.uint8)
    PR.write_png(path, img)
    with Image.open(path) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


# ------------------------------------------------------------------------------------------------ unpack_mask
def _pack_by_hand(mask, extra_tail_bits=False):
    """Words built bit by bit with Python integers: bit l of word w = linear pixel 64 w + l."""
    flat = mask.reshape(-1)
    words = [0] * ((flat.size + 63) // 64)
    for p in np.flatnonzero(flat):
        words[p // 64] |= 1 << (int(p) % 64)
    if extra_tail_bits and flat.size % 64:
        words[-1] |= ((1 << 64) - 1) & ~((1 << (flat.size % 64)) - 1)      # every bit beyond H*W set
    return np.array(words, dtype=np.uint64)


@pytest.mark.parametrize("H,W", [(8, 8), (64, 64), (100, 100), (37, 23)])       # H*W = 64, 4096, 10000 (16 bits in the last word), 851 (19)
def test_unpack_mask(H, W):
    rng = np.random.default_rng(H * W)
    mask = rng.random((H, W)) < 0.5
    mask[0, 0], mask[-1, -1] = True, True
    w = _pack_by_hand(mask)
    assert w.shape == ((H * W + 63) // 64,)
    for words in (w, w.view(np.int64)):
        got = metrics.unpack_mask(words, H, W)
        assert got.dtype == np.bool_ and got.shape == (H, W) and np.array_equal(got, mask)
    dirty = _pack_by_hand(mask, extra_tail_bits=True)
    assert np.array_equal(metrics.unpack_mask(dirty.view(np.int64), H, W), mask)                       # set bits beyond H*W are ignored
    other = ~mask
    batch = np.stack([w, _pack_by_hand(other)]).view(np.int64)
    got = metrics.unpack_mask(batch, H, W)
    assert got.shape == (2, H, W) and np.array_equal(got[0], mask) and np.array_equal(got[1], other)
    with pytest.raises(ValueError):
        metrics.unpack_mask(w[:-1] if w.size > 1 else np.zeros(2, np.uint64), H, W)
    with pytest.raises(ValueError):
        metrics.unpack_mask(w.astype(np.float64), H, W)


def test_unpack_mask_bit_order():
    got = metrics.unpack_mask(np.array([1 | (1 << 9) | (1 << 63)], dtype=np.uint64), 8, 8)
    want = np.zeros((8, 8), bool)
    want[0, 0] = want[1, 1] = want[7, 7] = True
    assert np.array_equal(got, want)
    assert np.array_equal(metrics.unpack_mask(np.array([-1], dtype=np.int64), 8, 8), np.ones((8, 8), bool))


# ------------------------------------------------------------------------------------------------ overlay
def test_overlay_blends_the_foreground_only():
    img = np.array([[[10.5, 200.25, 0.0], [255.0, 255.0, 255.0], [3.5, 4.5, 1.0]],
                    [[2.5, 3.5, 254.5], [100.4, 100.6, 300.0], [-4.0, 0.49, 0.5]]], dtype=np.float32)
    mask = np.array([[True, True, False], [False, True, False]])
    got = PR.overlay(img, mask)
    assert got.dtype == np.uint8 and got.shape == (2, 3, 3)
    # foreground: 0.5 * image + 0.5 * (255, 128, 0), half to even
    assert got[0, 0].tolist() == [133, 164, 0]          # 132.75, 164.125, 0
    assert got[0, 1].tolist() == [255, 192, 128]        # 255, 191.5 -> 192 (even), 127.5 -> 128 (even)
    assert got[1, 1].tolist() == [178, 114, 150]        # 177.7, 114.3, 150
    # background: the image, rounded half to even and clipped
    assert got[0, 2].tolist() == [4, 4, 1]              # 3.5 -> 4, 4.5 -> 4
    assert got[1, 0].tolist() == [2, 4, 254]            # 2.5 -> 2, 3.5 -> 4, 254.5 -> 254
    assert got[1, 2].tolist() == [0, 0, 0]              # -4 clipped; 0.49, 0.5 -> 0
    other = PR.overlay(img, mask, tint=(0, 0, 255), alpha=0.25)
    assert other[0, 0].tolist() == [8, 150, 64]         # 7.875, 150.1875, 63.75
    assert np.array_equal(other[~mask], got[~mask])
    clipped = PR.overlay(img, np.ones((2, 3), bool), tint=(0, 0, 0), alpha=0.0)
    assert clipped[1, 1].tolist() == [100, 101, 255]    # 300 clipped


# ------------------------------------------------------------------------------------------------ Gecko._evaluate with a stub learner
H = 16


def _masks_and_labels():
    rng = np.random.default_rng(9)
    masks = {i: rng.random((H, H)) < 0.4 for i in range(8)}
    masks[6][:] = False
    lab1 = rng.random((8, H, H)) < 0.4
    lab1[6] = False                                     # an empty mask against an empty label
    labels = np.stack([~lab1, lab1], axis=-1).astype(np.float32)
    return masks, labels


def _counts(p, l):
    return [int(np.count_nonzero(p & l)), int(np.count_nonzero(p | l)), int(np.count_nonzero(p)), int(np.count_nonzero(l))]


class _Stub:
    """The learner protocol as far as Gecko._evaluate uses it: mask_resident / score_resident / predict_resident hand out prepared masks
    (and the counts that go with them) and record their batches."""
    n_trainable = 1

    def __init__(self, masks, labels):
        self.masks, self.labels = masks, labels
        self.mask_calls, self.score_calls, self.predict_calls, self.steps = [], [], [], []

    def export_all(self):
        return {}

    def import_all(self, st):
        pass

    def load_task(self, x, y):
        pass

    def inner_step(self, idx, **kw):
        self.steps.append(list(idx))

    def _rows(self, idx):
        return np.asarray([_counts(self.masks[i], self.labels[i, ..., 1] > 0.5) for i in idx], dtype=np.int64)

    def score_resident(self, idx, training=False):
        assert training is False
        self.score_calls.append(list(idx))
        return self._rows(idx)

    def mask_resident(self, idx, training=False, counts=False, last_only=False):
        assert training is False and counts is True
        self.mask_calls.append((list(idx), last_only))
        keep = list(idx)[-1:] if last_only else list(idx)
        return np.stack([self.masks[i] for i in keep]), self._rows(keep)

    def predict_resident(self, idx, training=False):
        import torch
        assert training is False
        self.predict_calls.append(list(idx))
        p1 = np.stack([self.masks[i] for i in idx]).astype(np.float32)
        return torch.from_numpy(np.stack([1.0 - p1, p1], axis=-1))


class _NoMask(_Stub):
    mask_resident = None


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.mark.parametrize("transductive", [False, True])
def test_evaluate_saves_the_masks_and_keeps_the_ious(tmp_path, transductive):
    masks, labels = _masks_and_labels()
    train_idx, test_idx = [0, 1, 2, 3, 4], [5, 6, 7]
    images = np.random.default_rng(2).integers(0, 256, (8, H, H, 3)).astype(np.float32)
    res, trees, stubs = {}, {}, {}
    for dm in (True, False):
        for save in (False, True):
            L = _Stub(masks, labels)
            root = str(tmp_path / "dm{}_save{}".format(int(dm), int(save)))
            writer = PR.PredictionWriter(root, overlays=True) if save else None
            with contextlib.redirect_stdout(io.StringIO()):
                g = Gecko(L, transductive=transductive, device_metrics=dm, rng_mode="reference", dist=SingleRank(), prediction_writer=writer)
                res[dm, save] = g._evaluate(train_idx, test_idx, labels, inner_batch_size=4, inner_iters=2, replacement=False,
                                            task_name="some/task", eval_sample_num=3, images=images)
            trees[dm, save], stubs[dm, save] = _tree(root), L
    want = float(np.nanmean([metrics.iou(np.stack([~masks[t], masks[t]], -1).astype(np.float32), labels[t]) for t in test_idx]))
    assert res[True, True] == res[True, False] == res[False, True] == res[False, False] == want
    assert trees[True, False] == trees[False, False] == {}                               # no writer: nothing is written
    names = sorted(trees[True, True])
    assert names == sorted(os.path.join("some_task", "sample3_query{}_{}.png".format(j, kind)) for j in range(3) for kind in ("mask", "overlay"))
    assert trees[True, True] == trees[False, True]                                       # the two paths save the same files
    for j, t in enumerate(test_idx):
        stem = os.path.join(str(tmp_path / "dm1_save1"), "some_task", "sample3_query{}".format(j))
        assert np.array_equal(PR.read_png(stem + "_mask.png"), masks[t])
        assert np.array_equal(PR.read_png(stem + "_overlay.png"), PR.overlay(images[t], masks[t]))
    # the batches: one mask_resident call where the run without a writer calls score_resident, and nothing else
    L = stubs[True, True]
    batches = [test_idx] if transductive else [train_idx + [t] for t in test_idx]
    assert L.mask_calls == [(b, not transductive) for b in batches] and L.score_calls == [] and L.predict_calls == []
    assert stubs[True, False].score_calls == batches and stubs[True, False].mask_calls == []
    for save in (False, True):                                                           # the default path: no extra device work
        assert stubs[False, save].predict_calls == batches and stubs[False, save].mask_calls == [] and stubs[False, save].score_calls == []


def test_writer_names_and_switches(tmp_path):
    masks, labels = _masks_and_labels()
    root = str(tmp_path / "w")
    L = _Stub(masks, labels)
    with contextlib.redirect_stdout(io.StringIO()):
        g = Gecko(L, transductive=True, device_metrics=True, rng_mode="reference", dist=SingleRank(),
                  prediction_writer=PR.PredictionWriter(root))                          # overlays off; eval_sample_num None -> sample0
        g._evaluate([0, 1], [5, 7], labels, inner_batch_size=2, inner_iters=1, replacement=False, task_name="t",
                    images=np.zeros((8, H, H, 3), np.float32))
        # the early-stopping site never saves
        g._early_stopping_learn([0, 1], [5, 7], labels, 2, min_steps=1, max_steps=2, replacement=False, lr=1e-3)
    assert sorted(_tree(root)) == [os.path.join("t", "sample0_query0_mask.png"), os.path.join("t", "sample0_query1_mask.png")]
    assert len(L.mask_calls) == 1 and len(L.score_calls) == 2
    w = PR.PredictionWriter(root, overlays=True)
    w.save("a/b\\c", None, 4, masks[0])                                                 # overlays on but no image: the mask alone
    assert os.path.exists(os.path.join(root, "a_b_c", "sample0_query4_mask.png")) and len(os.listdir(os.path.join(root, "a_b_c"))) == 1
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="mask_resident"):
            Gecko(_NoMask(masks, labels), device_metrics=True, dist=SingleRank(), prediction_writer=w)
        with pytest.raises(ValueError, match="mask_resident"):
            FOMLIS(_Stub(masks, labels), lanes=[_NoMask(masks, labels)], device_metrics=True, dist=SingleRank(), prediction_writer=w)
        assert Gecko(_NoMask(masks, labels), dist=SingleRank(), prediction_writer=w).prediction_writer is w      # the host path needs nothing new
        assert Gecko(_NoMask(masks, labels), device_metrics=True, dist=SingleRank()).prediction_writer is None


def test_evaluate_hands_the_sample_number_to_the_lanes(tmp_path):
    """Gecko.evaluate over two lanes (_evaluate_concurrently): the files carry eval_sample_num and the task names."""
    import torch
    from mliis_amd.metaseg import DeviceTask
    masks, labels = _masks_and_labels()
    x = torch.zeros(8, H, H, 3)
    tasks = [DeviceTask("t%d" % i, x, torch.from_numpy(labels)) for i in range(2)]
    out = {}
    for lanes in (0, 1):
        root = str(tmp_path / str(lanes))
        L = _Stub(masks, labels)
        random.seed(3)                                  # (the train / test split is drawn from the global generator)
        with contextlib.redirect_stdout(io.StringIO()):
            g = Gecko(L, transductive=True, device_metrics=True, rng_mode="reference", dist=SingleRank(),
                      lanes=[_Stub(masks, labels)] * lanes, prediction_writer=PR.PredictionWriter(root))
            res = g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=1, eval_all_tasks=True, test_shots=3, eval_sample_num=2)
        out[lanes] = (res, _tree(root))
    assert out[0] == out[1]
    assert sorted(out[1][1]) == sorted(os.path.join("t%d" % i, "sample2_query%d_mask.png" % j) for i in range(2) for j in range(3))


# ------------------------------------------------------------------------------------------------ flags
def test_flags_and_the_environment_switch():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.save_predictions is None and off.save_prediction_overlays is False
    assert A.prediction_writer(off, environ={}) is None
    assert A.prediction_writer(off, environ={"SAVE_PREDICTIONS": ""}) is None
    w = A.prediction_writer(p.parse_args(["--save-predictions", "out/dir"]), environ={})
    assert isinstance(w, PR.PredictionWriter) and (w.directory, w.overlays) == ("out/dir", False)
    w = A.prediction_writer(p.parse_args(["--save-predictions", "d", "--save-prediction-overlays"]), environ={})
    assert (w.directory, w.overlays) == ("d", True)
    w = A.prediction_writer(off, environ={"SAVE_PREDICTIONS": "1"})                     # the reference's switch and directory
    assert (w.directory, w.overlays) == ("predictions", True)
    w = A.prediction_writer(p.parse_args(["--save-predictions", "mine"]), environ={"SAVE_PREDICTIONS": "1"})
    assert (w.directory, w.overlays) == ("mine", True)                                  # an explicit flag wins
    # the reference's parser does not know the flags; the evaluation keywords shared with the search and the k-shot curves carry no writer
    ref = A.argument_parser(extensions=False)
    assert not hasattr(ref.parse_args([]), "save_predictions") and not hasattr(ref.parse_args([]), "save_prediction_overlays")
    for flag in (["--save-predictions", "d"], ["--save-prediction-overlays"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            ref.parse_args(flag)
    assert A.prediction_writer(ref.parse_args([]), environ={}) is None
    assert "prediction_writer" not in A.evaluate_kwargs(p.parse_args(["--save-predictions", "d"]))
    assert "prediction_writer" not in A.train_kwargs(p.parse_args(["--save-predictions", "d"]))


def test_environment_switch_is_read_from_the_process(monkeypatch):
    off = A.argument_parser().parse_args([])
    monkeypatch.delenv("SAVE_PREDICTIONS", raising=False)
    assert A.prediction_writer(off) is None
    monkeypatch.setenv("SAVE_PREDICTIONS", "1")
    w = A.prediction_writer(off)
    assert (w.directory, w.overlays) == ("predictions", True)


def test_only_evaluate_gecko_hands_the_writer_on():
    from mliis_amd import eval as E
    seen = []

    class Meta:
        dist = SingleRank()

        def __init__(self, learner, **kw):
            seen.append(kw)

        def evaluate(self, dataset, **kw):
            return 0.5, {"t": 0.5}

        def evaluate_m_k_shot_ranges_all_tasks(self, **kw):
            return [1], [0.5]

    w = PR.PredictionWriter("unused")
    with contextlib.redirect_stdout(io.StringIO()):
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta, prediction_writer=w)
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta)
        E.run_k_shot_learning_curves_experiment(object(), [], num_samples=1, meta_fn=Meta, csv_outpath=None, prediction_writer=w)
    assert [kw.get("prediction_writer") for kw in seen] == [w, None, None] and "prediction_writer" not in seen[1]
