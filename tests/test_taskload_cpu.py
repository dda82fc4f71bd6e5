"""Byte-resident tasks, the host side: metaseg.expand_bytes_host (the numpy restatement of csrc/taskload.hip) against
tfrecord.parse_example and against torch's bilinear resize, metaseg.ByteTask and its views, tfrecord.parse_example_u8 / ShardTask's byte
mode, the --resident-dataset / --stored-image-size flags, and libmliis_data.so's exported ABI against include/mliis_data.h."""
import contextlib
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mliis_amd import args as A
from mliis_amd import metaseg, tfrecord
from mliis_amd.reptile import _to_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESAMPLE_SHAPES = [((5, 7), (8, 12)), ((4, 4), (8, 8)), ((8, 8), (5, 5)), ((1, 3), (4, 6))]


def _pool(n, h, w, seed=0):
    g = np.random.default_rng(seed)
    images = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    masks = g.integers(0, 256, (n, h, w), dtype=np.uint8)
    flat = masks.reshape(-1)
    k = min(256, flat.size)
    flat[:k] = np.arange(k, dtype=np.uint8)          # every byte value when the pool has room for them
    return images, masks


def test_byte_quotients_are_the_correctly_rounded_ones():
    """numpy's float32 division by 255 -- what parse_example does -- is the correctly rounded k / 255 for all 256 bytes."""
    k = np.arange(256)
    got = (np.stack([255 - k, k]).astype(np.float32) / 255.0)
    want = (np.stack([255 - k, k]).astype(np.float64) / 255.0).astype(np.float32)     # one rounding of the exact quotient's double
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_same_size_equals_parse_example_bit_for_bit(tmp_path):
    H = 16
    images, masks = _pool(3, H, H)
    assert set(np.unique(masks)) == set(range(256))
    path = str(tmp_path / "t.tfrecord.gzip")
    tfrecord.write_records(path, [tfrecord.make_example_bytes(i, m) for i, m in zip(images, masks)])
    records = list(tfrecord.read_records(path))
    pairs = [tfrecord.parse_example(r, H) for r in records]
    x_ref, y_ref = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    raw = [tfrecord.parse_example_u8(r, H) for r in records]
    xb, mb = np.stack([p[0] for p in raw]), np.stack([p[1] for p in raw])
    assert xb.dtype == np.uint8 and mb.dtype == np.uint8 and np.array_equal(xb, images) and np.array_equal(mb, masks)
    x, y = metaseg.expand_bytes_host(xb, mb, H, H)
    assert x.dtype == np.float32 and y.dtype == np.float32
    assert x.tobytes() == x_ref.tobytes() and y.tobytes() == y_ref.tobytes()
    with pytest.raises(ValueError):
        tfrecord.parse_example_u8(records[0], H + 1)


@pytest.mark.parametrize("src,dst", RESAMPLE_SHAPES)
def test_resampling_matches_torch_bilinear_and_the_integer_nearest_rule(src, dst):
    (h, w), (H, W) = src, dst
    images, masks = _pool(3, h, w, seed=h * 100 + w)
    x64, y64 = metaseg.expand_bytes_host(images, masks, H, W, dtype=np.float64)
    ref = F.interpolate(torch.from_numpy(images.astype(np.float64)).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                        align_corners=False).permute(0, 2, 3, 1).numpy()
    err = float(np.abs(x64 - ref).max())
    print("max |expand_bytes_host(float64) - torch bilinear| {} -> {}: {:.3e}".format(src, dst, err))
    assert x64.dtype == np.float64 and x64.shape == (3, H, W, 3) and err <= 1e-10
    # nearest at half-pixel centres in integers, written out pixel by pixel
    want = np.zeros((3, H, W), dtype=np.uint8)
    for i in range(H):
        for j in range(W):
            want[:, i, j] = masks[:, ((2 * i + 1) * h) // (2 * H), ((2 * j + 1) * w) // (2 * W)]
    y_want = np.stack([255 - want, want], axis=-1).astype(np.float32) / 255.0
    x32, y32 = metaseg.expand_bytes_host(images, masks, H, W)
    assert y32.dtype == np.float32 and y32.tobytes() == y_want.tobytes() and np.array_equal(y64, y_want.astype(np.float64))
    assert x32.dtype == np.float32 and float(np.abs(x32 - x64).max()) <= 255 * 8 * 2.0 ** -24
    assert metaseg.expand_bytes_host(None, masks, H, W)[0] is None and metaseg.expand_bytes_host(images, None, H, W)[1] is None


def test_byte_task_views_behave_like_the_arrays_they_stand_for():
    H = 6
    images, masks = _pool(5, H, H, seed=3)
    task = metaseg.ByteTask("t", images, masks, H)
    assert task.name == "t" and task.batch_size == 5 and task.stored_size == (H, H)
    x_all, y_all = metaseg.expand_bytes_host(images, masks, H, H)
    x, y = task.sample(3)
    assert x.shape == (3, H, H, 3) and y.shape == (3, H, H, 2) and len(x) == 3 and len(y) == 3
    assert not hasattr(x, "detach") and not torch.is_tensor(x) and x.is_prefix()
    assert np.array_equal(np.asarray(x), x_all[:3]) and np.array_equal(np.asarray(y), y_all[:3])       # the FIRST three
    assert np.asarray(x).dtype == np.float32 and np.asarray(x) is np.asarray(x)                           # expanded once per view
    assert np.array_equal(_to_numpy(y), y_all[:3])
    assert x[1].shape == (H, H, 3) and np.array_equal(np.asarray(x[1]), x_all[1]) and np.array_equal(_to_numpy(y[2]), y_all[2])
    assert x[1:3].shape == (2, H, H, 3) and np.array_equal(np.asarray(y[1:3]), y_all[1:3]) and not x[1:3].is_prefix()
    sel = [2, 0, 2]
    assert x[sel].shape == (3, H, H, 3) and len(y[sel]) == 3 and np.array_equal(np.asarray(x[sel]), x_all[sel])
    assert np.array_equal(np.asarray(y[np.array(sel)]), y_all[sel])
    assert np.array_equal(np.asarray(x)[sel], x_all[sel])                                              # and numpy indexing after conversion
    assert np.array_equal(np.stack([np.asarray(v) for v in y]), y_all[:3])
    # sample_task treats it as it treats a DeviceTask (first num_shots examples, clipped to the pool with a warning)
    (sx, sy), name = metaseg.sample_task([task], 4, None, return_task_name=True)
    assert name == "t" and sx.shape == (4, H, H, 3) and np.array_equal(np.asarray(sy), y_all[:4])
    with pytest.warns(UserWarning):
        (sx, _) = metaseg.sample_task([task], 9)
    assert sx.shape == (5, H, H, 3)
    with pytest.raises(ValueError):
        metaseg.ByteTask("f", images.astype(np.float32), masks, H)
    with pytest.raises(ValueError):
        metaseg.ByteTask("s", images, masks[:, :-1], H)


def test_a_view_of_a_task_stored_at_another_size_reports_the_expanded_shape():
    images, masks = _pool(4, 5, 5, seed=4)
    task = metaseg.ByteTask("t", torch.from_numpy(images), torch.from_numpy(masks), 8)
    x, y = task.sample(2)
    assert task.stored_size == (5, 5) and x.shape == (2, 8, 8, 3) and y.shape == (2, 8, 8, 2) and x[0].shape == (8, 8, 3)
    xe, ye = metaseg.expand_bytes_host(images[:2], masks[:2], 8, 8)
    assert np.array_equal(np.asarray(x), xe) and np.array_equal(np.asarray(y), ye) and np.array_equal(np.asarray(y[1]), ye[1])


def test_synthetic_bytes_expand_to_the_synthetic_floats():
    for size in (16, 20):
        xb, mb = metaseg.synthetic_task_bytes(3, size, seed=5)
        x_ref, y_ref = metaseg.synthetic_task(3, size, seed=5)
        x, y = metaseg.expand_bytes_host(xb, mb, size, size)
        assert xb.dtype == np.uint8 and mb.dtype == np.uint8 and set(np.unique(mb)) <= {0, 255}
        assert x.tobytes() == x_ref.tobytes() and y.tobytes() == y_ref.tobytes()


def _write_shards(data_dir, H, n_tasks=4, examples=3, seed=0):
    os.makedirs(data_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    names = tfrecord.fss_test_task_ids()[:2] + ["zz_train_task_%d" % i for i in range(n_tasks - 2)]
    arrays = {}
    for name in names:
        imgs = rng.integers(0, 256, size=(examples, H, H, 3), dtype=np.uint8)
        msks = rng.integers(0, 256, size=(examples, H, H), dtype=np.uint8)
        tfrecord.write_records(os.path.join(data_dir, name + ".tfrecord.gzip"), [tfrecord.make_example_bytes(i, m) for i, m in zip(imgs, msks)])
        arrays[name + ".tfrecord.gzip"] = (imgs, msks)
    return arrays


def test_shard_tasks_default_to_host_floats_and_can_keep_bytes(tmp_path):
    H = 8
    data_dir = str(tmp_path / "fss")
    arrays = _write_shards(data_dir, H)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = tfrecord.read_fss_1000_dataset(data_dir, image_size=H)
        same = tfrecord.read_fss_1000_dataset(data_dir, image_size=H, resident=None)
        kept = tfrecord.read_fss_1000_dataset(data_dir, image_size=H, resident="cpu")
        big = tfrecord.read_fss_1000_dataset(data_dir, image_size=12, resident="cpu", stored_size=H)
    assert len(plain) == 6 and [len(p) for p in plain] == [len(p) for p in same] and plain[3:] == same[3:] == kept[3:]
    for a, b, c, d in zip(plain[0] + plain[2], same[0] + same[2], kept[0] + kept[2], big[0] + big[2]):
        assert a.name == b.name == c.name == d.name and a.batch_size == c.batch_size == 3
        (xa, ya), (xb, yb), (xc, yc), (xd, yd) = a.sample(2), b.sample(2), c.sample(2), d.sample(2)
        assert isinstance(xa, np.ndarray) and isinstance(xb, np.ndarray) and xa.dtype == np.float32        # today's return values
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
        assert isinstance(xc, metaseg.ByteView) and xc.shape == xa.shape and yc.shape == ya.shape
        assert np.asarray(xc).tobytes() == xa.tobytes() and np.asarray(yc).tobytes() == ya.tobytes()
        imgs, msks = arrays[a.name]
        xe, ye = metaseg.expand_bytes_host(imgs[:2], msks[:2], 12, 12)
        assert xd.shape == (2, 12, 12, 3) and np.array_equal(np.asarray(xd), xe) and np.array_equal(np.asarray(yd), ye)
        with pytest.raises(ValueError):
            c.sample(4)
    with pytest.raises(ValueError, match="--resident-dataset"), contextlib.redirect_stdout(io.StringIO()):
        tfrecord.read_fss_1000_dataset(data_dir, image_size=12, stored_size=H)
    with contextlib.redirect_stdout(io.StringIO()):
        tasks, names = tfrecord.read_fp_k_shot_dataset(data_dir, all_task_names=[{"zz_train_task_0"}], image_size=12, resident="cpu", stored_size=H)
    assert names == ["zz_train_task_0"] and tasks[0].sample(3)[1].shape == (3, 12, 12, 2)


def test_flags_default_off_and_the_stored_size_refusal():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.resident_dataset is False and off.stored_image_size is None and A.stored_image_size(off) == off.image_size
    ref = A.argument_parser(extensions=False)
    for flag in (["--resident-dataset"], ["--stored-image-size", "48"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            ref.parse_args(flag)
    assert A.stored_image_size(ref.parse_args(["--image_size", "96"])) == 96
    on = p.parse_args(["--resident-dataset", "--stored-image-size", "48", "--image_size", "64"])
    assert on.resident_dataset is True and A.stored_image_size(on) == 48
    # the keyword builders do not see the flags: same dictionaries with and without them
    base = p.parse_args(["--image_size", "64"])

    def kw(fn, a):
        return {k: (v.func, v.keywords) if hasattr(v, "func") else v for k, v in fn(a).items()}
    for fn in (A.model_kwargs, A.train_kwargs, A.evaluate_kwargs):
        assert kw(fn, on) == kw(fn, base)
        assert kw(fn, off) == kw(fn, ref.parse_args([]))
    assert A.stored_image_size(p.parse_args(["--stored-image-size", "64", "--image_size", "64"])) == 64
    with pytest.raises(ValueError, match="--resident-dataset"):
        A.stored_image_size(p.parse_args(["--stored-image-size", "48", "--image_size", "64"]))
    with pytest.raises(ValueError):
        A.stored_image_size(p.parse_args(["--stored-image-size", "0", "--resident-dataset"]))


def test_main_refuses_a_stored_size_it_cannot_serve_before_building_anything():
    import run_metasegnet

    def no_learner(**kw):
        raise AssertionError("the learner was built")
    with pytest.raises(ValueError, match="--resident-dataset"), contextlib.redirect_stdout(io.StringIO()):
        run_metasegnet.main(["--image_size", "64", "--stored-image-size", "48", "--synthetic-tasks", "4"], learner_factory=no_learner, device="cpu")


def test_data_library_exports_its_header_and_nothing_else():
    """libmliis_data.so (csrc/taskload.hip) against include/mliis_data.h: its dynamic symbols are the header's declarations, the ctypes table
    has their argument counts, and none of them belongs to the other two libraries' C ABIs."""
    from mliis_amd import _lib
    if not os.path.exists(_lib.DATA_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_data.h")).read(), flags=re.S)
    decls = {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
             for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.DATA_LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(decls) == set(_lib.DATA_SIGNATURES) == syms == {"mliis_data_last_error", "mliis_task_expand_u8"}
    for name, params in decls.items():
        assert len(params) == len(_lib.DATA_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES))
    assert _lib.data_lib.load().mliis_data_last_error() == b""
