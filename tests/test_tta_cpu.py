"""Flip test-time augmentation at evaluation without a GPU: the views' names and order, the flag, the driver's refusal on a learner without
the keyword, the meta-learner's scoring sites driven by a recording learner, libmliis_tta.so against its header (in tree and from a clean
out-of-tree build), and the float64 reference's own consistency (tests/tta_ref.py)."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import tta_ref as R
from mliis_amd import args as A
from mliis_amd import metrics as M
from mliis_amd import views as V
from mliis_amd.metaseg import DeviceTask
from mliis_amd.reptile import FOMLIS, Gecko, SingleRank
from test_build_cpu import _affected_packed_forms, _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_tta_last_error", "mliis_view_gather", "mliis_view_merge"}


# ------------------------------------------------------------------------------------------------ views and flags
def test_views_are_canonicalised_and_refused():
    assert V.VIEWS == R.ORDER and V.FLIPS == R.FLIPS            # the tests' restatement names the same mirrors
    assert V.canonical(()) == () and V.canonical(None) == () and V.canonical("vflip") == ("vflip",)
    assert V.canonical(["hvflip", "hflip"]) == ("hflip", "hvflip") and V.canonical(("hvflip", "vflip", "hflip")) == V.VIEWS
    for bad in (["rot90"], ["hflip", "hflip"], ["identity"], [""]):
        with pytest.raises(ValueError):
            V.canonical(bad)
    # hflip mirrors the columns like np.fliplr of an image, vflip the rows
    z = np.arange(2 * 3 * 4 * 2).reshape(2, 3, 4, 2)
    assert np.array_equal(R.flip_np(z, "hflip")[1], np.fliplr(z[1])) and np.array_equal(R.flip_np(z, "vflip")[0], np.flipud(z[0]))
    assert np.array_equal(R.flip_np(z, "hvflip"), R.flip_np(R.flip_np(z, "hflip"), "vflip"))


def test_flag_parses_refuses_and_leaves_the_keyword_tables_alone():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.eval_tta is None and A.eval_views(off) == ()
    assert A.eval_views(p.parse_args(["--eval-tta", "hflip"])) == ("hflip",)
    on = p.parse_args(["--eval-tta", "hvflip", "hflip", "--device-metrics"])
    assert A.eval_views(on) == ("hflip", "hvflip") and on.device_metrics is True
    assert A.eval_views(p.parse_args(["--eval-tta", "hvflip", "vflip", "hflip"])) == ("hflip", "vflip", "hvflip")
    with pytest.raises(ValueError, match="more than once"):
        A.eval_views(p.parse_args(["--eval-tta", "hflip", "vflip", "hflip"]))
    for bad in (["--eval-tta", "rot90"], ["--eval-tta"], ["--eval-tta", "hflip", "transpose"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            p.parse_args(bad)
    b = p.parse_args(["--device-metrics"])      # only the final passes merge views: nothing reaches the keyword tables of the other drivers
    assert A.evaluate_kwargs(on) == A.evaluate_kwargs(b) and not any("view" in k or "tta" in k for k in A.evaluate_kwargs(on))
    ta, tb = A.train_kwargs(on), A.train_kwargs(b)
    assert {k: v for k, v in ta.items() if k != "meta_fn"} == {k: v for k, v in tb.items() if k != "meta_fn"} and ta["meta_fn"] is tb["meta_fn"]
    assert A.model_kwargs(on) == A.model_kwargs(b)
    ref = A.argument_parser(extensions=False)
    assert not hasattr(ref.parse_args([]), "eval_tta") and A.eval_views(ref.parse_args([])) == ()
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        ref.parse_args(["--eval-tta", "hflip"])


def _oracle_factory(**kw):
    from oracle import efficientlab_ref as Ref
    torch.set_num_threads(4)
    return Ref.OracleLearner(name="efficientnet-b0", image_size=32, rsd=(2, 4), seed=0, dtype=torch.float32, lr=1e-3, l2=False, dice=False,
                             label_smoothing=0.0, drop_connect=False)


def test_main_refuses_views_on_a_learner_without_the_keyword_before_training(tmp_path):
    import run_metasegnet
    base = ["--image_size", "32", "--rsd", "2", "4", "--sgd", "--shots", "2", "--synthetic-tasks", "6", "--meta-iters", "1", "--checkpoint",
            str(tmp_path / "ckpt")]
    buf = io.StringIO()
    with pytest.raises(ValueError, match="views="), contextlib.redirect_stdout(buf):
        run_metasegnet.main(base + ["--eval-tta", "hflip"], learner_factory=_oracle_factory, device="cpu")
    assert "Meta-training..." not in buf.getvalue() and not os.path.exists(str(tmp_path / "ckpt"))

    def no_learner(**kw):
        raise AssertionError("the learner was built")
    with pytest.raises(ValueError, match="more than once"), contextlib.redirect_stdout(io.StringIO()):
        run_metasegnet.main(base + ["--eval-tta", "vflip", "vflip"], learner_factory=no_learner, device="cpu")


def test_the_driver_passes_the_views_only_when_set():
    from mliis_amd import eval as E
    seen = []

    class Meta:
        dist = SingleRank()

        def __init__(self, learner, **kw):
            seen.append(kw)

        def evaluate(self, dataset, **kw):
            return 0.5, {"t": 0.5}

    with contextlib.redirect_stdout(io.StringIO()):
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta, eval_views=("hflip", "vflip"))
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta)
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta, eval_views=())
    assert seen[0]["eval_views"] == ("hflip", "vflip") and "eval_views" not in seen[1] and "eval_views" not in seen[2]


# ------------------------------------------------------------------------------------------------ the meta-learner's scoring sites
HF = 4


class _Recorder:
    """The learner protocol as far as Gecko's evaluation uses it; every scoring call is recorded with the views it was given."""
    n_trainable = 1
    optimizer = "sgd"

    def __init__(self):
        self.calls = []

    def export_all(self):
        return {}

    def import_all(self, st):
        pass

    def load_task(self, x, y):
        self.n = int(x.shape[0])

    def inner_step(self, idx, **kw):
        pass

    def _seen(self, what, idx, views, last_only=False):
        assert isinstance(views, tuple)
        self.calls.append((what, len(idx), views))
        return 1 if last_only else len(idx)

    def predict_resident(self, idx, training=False, views=()):
        n = self._seen("predict", idx, views)
        return torch.zeros(n, HF, HF, 2)

    def score_resident(self, idx, training=False, views=()):
        return np.ones((self._seen("score", idx, views), 4), dtype=np.int64)

    def mask_resident(self, idx, training=False, counts=False, last_only=False, views=()):
        n = self._seen("mask", idx, views, last_only)
        m = np.zeros((n, HF, HF), dtype=bool)
        return (m, np.ones((n, 4), dtype=np.int64)) if counts else m

    def histogram_resident(self, idx, training=False, last_only=False, masks=False, views=()):
        n = self._seen("hist", idx, views, last_only)
        h = np.ones((n, 2, M.HIST_BINS), dtype=np.int64)
        return (h, np.zeros((n, HF, HF), dtype=bool)) if masks else h


class _NoViews(_Recorder):
    def score_resident(self, idx, training=False):
        return np.ones((len(idx), 4), dtype=np.int64)


class _Swallows(_Recorder):
    def predict_resident(self, idx, training=False, **kw):
        return torch.zeros(len(idx), HF, HF, 2)


class _Writer:
    overlays = False

    def save(self, task, sample, j, mask, image=None):
        pass


def _tasks():
    y = torch.zeros(9, HF, HF, 2)
    y[..., 0] = 1.0
    return [DeviceTask("t%d" % i, torch.zeros(9, HF, HF, 3), y.clone()) for i in range(2)]


PATHS = {"predict": {}, "score": {"device_metrics": True}, "mask": {"device_metrics": True, "prediction_writer": _Writer()},
         "hist": {"device_metrics": True, "threshold_sweep": lambda *a: None}}


@pytest.mark.parametrize("transductive", [False, True])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_evaluate_passes_the_views_at_every_scoring_site(path, transductive):
    for views, lanes in (((), 0), (("vflip", "hflip"), 0), (("hvflip",), 1)):
        L, Ls = _Recorder(), [_Recorder() for _ in range(lanes)]
        with contextlib.redirect_stdout(io.StringIO()):
            g = Gecko(L, transductive=transductive, rng_mode="reference", dist=SingleRank(), lanes=Ls, eval_views=views, **PATHS[path])
            assert g.eval_views == V.canonical(views)
            g.evaluate(_tasks(), num_shots=5, inner_batch_size=4, inner_iters=2, eval_all_tasks=True, test_shots=4)
        calls = L.calls + [c for ln in Ls for c in ln.calls]
        per_task = 1 if transductive else 4
        assert len(calls) == 2 * per_task and all(c == (path, 4 if transductive else 6, V.canonical(views)) for c in calls), calls
        if lanes:
            assert L.calls and Ls[0].calls                      # one task each


def test_early_stopping_and_the_k_shot_curves_pass_no_views():
    L = _Recorder()
    task = _tasks()[0]
    with contextlib.redirect_stdout(io.StringIO()):
        for kw in ({}, {"device_metrics": True}):
            g = Gecko(L, rng_mode="reference", dist=SingleRank(), eval_views=("hflip",), **kw)
            L.load_task(task.images, task.labels)
            g._early_stopping_learn([0, 1, 2, 3], [4, 5], task.labels, 2, 0, 3, False)
            g.evaluate_k_shot_range(task, k_range=[2, 3], iter_range=[1, 1], test_samples=2, esimate_inner_iters_with_early_stoppping=False,
                                    inner_batch_size=2, replacement=False)
            g.evaluate_with_early_stopping([task], num_shots=4, inner_batch_size=2, max_steps=2, eval_all_tasks=True, test_shots=2)
    assert L.calls and all(views == () for _, _, views in L.calls), L.calls
    # the drivers of the search and of the k-shot curves build their meta-learner without views (and so do the training-time evaluations)
    import inspect
    from mliis_amd import eval as E
    from mliis_amd import train as T
    for fn in (E.optimize_update_hyperparams, E.run_k_shot_learning_curves_experiment):
        assert "eval_views" not in inspect.getsource(fn)
    assert "eval_views" not in inspect.getsource(T)


def test_views_need_a_learner_with_the_keyword():
    with contextlib.redirect_stdout(io.StringIO()):
        for cls in (Gecko, FOMLIS):
            with pytest.raises(ValueError, match="views="):
                cls(_NoViews(), dist=SingleRank(), eval_views=("hflip",))
        with pytest.raises(ValueError, match="views="):
            Gecko(_Recorder(), lanes=[_NoViews()], dist=SingleRank(), eval_views=("hflip",))
        with pytest.raises(ValueError, match="views="):
            Gecko(_Swallows(), dist=SingleRank(), eval_views=("hflip",))        # a **kwargs would drop the views silently
        with pytest.raises(ValueError, match="unknown"):
            Gecko(_Recorder(), dist=SingleRank(), eval_views=("rot90",))
        with pytest.raises(ValueError, match="more than once"):
            Gecko(_Recorder(), dist=SingleRank(), eval_views=("hflip", "hflip"))
        assert Gecko(_NoViews(), dist=SingleRank()).eval_views == ()             # the default needs nothing new
        assert Gecko(_NoViews(), dist=SingleRank(), eval_views=()).eval_views == ()
    from oracle import efficientlab_ref as Ref
    assert not V.accepts_views(Ref.OracleLearner.predict_resident)


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_tta.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_tta_library(tmp_path):
    """A clean out-of-tree build of the library's target: one translation unit built without the SLP vectoriser, the shared export map,
    exactly the header's names as dynamic symbols, a gfx950 code object only, none of the packed fp32 forms; the in-tree library is not
    disturbed.  (tests/test_build_cpu.py builds `all` out of tree and counts one object per .hip file, this one included.)"""
    build = str(tmp_path / "obj")
    intree = os.path.join(ROOT, "mliis_amd", "libmliis_tta.so")
    before = os.path.getmtime(intree) if os.path.exists(intree) else None
    so = os.path.join(build, "libmliis_tta.so")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, so], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(so) and sorted(f for f in os.listdir(build) if f.endswith(".o")) == ["tta.o"]
    line = next(ln for ln in r.stdout.splitlines() if " tta.hip " in ln + " ")
    assert "-fno-slp-vectorize" in line and "--offload-arch=gfx950" in line
    assert any("--version-script=exports.map" in ln and "libmliis_tta.so" in ln for ln in r.stdout.splitlines())
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    assert (os.path.getmtime(intree) if os.path.exists(intree) else None) == before
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(TTA_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(TTA_OBJS\) \$\(TTA_TARGET\)", mk)
    assert re.search(r"^\$\(BUILD\)/tta\.o: CXXFLAGS \+= -fno-slp-vectorize", mk, flags=re.M)


def test_tta_library_exports_its_header_and_refuses_bad_arguments_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.TTA_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.TTA_SIGNATURES) == set(_dynamic_symbols(_lib.TTA_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.TTA_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES) |
                             set(_lib.LAYERLOG_SIGNATURES) | set(_lib.CLIP_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.LOSS_SIGNATURES))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_packed_forms import affected_kernels
    assert affected_kernels(_lib.TTA_LIB_PATH) == {}
    lib = _lib.tta_lib
    err = lib.load().mliis_tta_last_error
    assert err() == b""
    ARG, UNSUPPORTED, ALIGN = -1, -2, -3
    # nothing is launched for any of these: the pointers are never dereferenced on the host and no device is needed to refuse them
    g = lib.load().mliis_view_gather
    assert g(None, None, 1, 4, 4, 3, 0, 1, 4096, None) == ARG and err().startswith(b"view_gather: null")
    assert g(4096, None, 1, 4, 4, 3, 0, 1, None, None) == ARG
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert g(4096, None, n, h, w, 3, 0, 1, 8192, None) == ARG
    assert g(4096, None, 1, 4, 4, 5, 0, 1, 8192, None) == ARG and b"channels" in err()
    assert g(4096, None, 1, 4, 4, 0, 0, 1, 8192, None) == ARG
    assert g(4096, None, 1, 4, 4, 3, 0, 1, 4096, None) == ARG and b"overlaps" in err()            # dst == src
    assert g(4096, None, 1, 4, 4, 3, 0, 0, 4096 + 4 * 47, None) == ARG                             # dst inside src's last word
    assert g(4096, None, 65536, 256, 256, 4, 0, 1, 1 << 40, None) == UNSUPPORTED
    assert g(4098, None, 1, 4, 4, 3, 0, 1, 8192, None) == ALIGN and g(4096, None, 1, 4, 4, 3, 0, 1, 8193, None) == ALIGN
    assert g(4096, 6, 1, 4, 4, 3, 0, 1, 8192, None) == ALIGN and b"aligned" in err()
    m = lib.load().mliis_view_merge
    assert m(None, 4096, 8192, 1, 4, 4, 2, 0, 1, 0.5, None) == ARG and err().startswith(b"view_merge: null")
    assert m(12288, 4096, None, 1, 4, 4, 2, 0, 1, 0.5, None) == ARG
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert m(12288, 4096, 8192, n, h, w, 2, 0, 1, 0.5, None) == ARG
    assert m(12288, 4096, 8192, 1, 4, 4, 5, 0, 1, 0.5, None) == ARG
    for scale in (0.0, -0.5, float("inf"), float("-inf"), float("nan")):
        assert m(12288, 4096, 8192, 1, 4, 4, 2, 0, 1, scale, None) == ARG and b"scale" in err(), scale
    assert m(8192, 4096, 8192, 1, 4, 4, 2, 0, 1, 0.5, None) == ARG and b"overlaps b" in err()      # dst == b
    assert m(8192, None, 8192, 1, 4, 4, 2, 0, 0, 0.5, None) == ARG
    assert m(4096 + 8, 4096, 8192, 1, 4, 4, 2, 0, 1, 0.5, None) == ARG and b"overlaps a" in err()  # a shifted a is not the in-place form
    assert m(12288, 4096, 8192, 65536, 256, 256, 4, 0, 1, 0.5, None) == UNSUPPORTED
    assert m(12290, 4096, 8192, 1, 4, 4, 2, 0, 1, 0.5, None) == ALIGN and m(12288, 4097, 8192, 1, 4, 4, 2, 0, 1, 0.5, None) == ALIGN


def test_the_library_is_loaded_by_build_and_by_nothing_without_views():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "tta_lib.load()" in src
    code = ("import mliis_amd, mliis_amd.ops, mliis_amd.learner, mliis_amd.reptile, mliis_amd.eval, mliis_amd.args, run_metasegnet, "
            "mliis_amd._lib as L; assert L.tta_lib._dll is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
    # the only users: the two wrappers of ops, reached from Learner._forward_views alone
    ops_src = open(os.path.join(ROOT, "mliis_amd", "ops.py")).read()
    assert len(re.findall(r"tta_lib\.", ops_src)) == 2
    learner_src = open(os.path.join(ROOT, "mliis_amd", "learner.py")).read()
    assert "tta_lib" not in learner_src and learner_src.count("ops.view_gather(") == 1 and learner_src.count("ops.view_merge(") == 2


# ------------------------------------------------------------------------------------------------ the float64 reference against itself
def test_reference_flips_commute_with_the_align_corners_resize():
    """What the design rests on, in float64: resizing a mirrored map is mirroring the resized map (to rounding), so averaging at decoder
    resolution and resizing once equals the reference's average at full resolution; the fp32 restatement stays within tau / 4 of it."""
    rng = np.random.default_rng(5)
    z = rng.normal(0.0, 3.0, (2, 7, 5, 2))
    for v in R.ORDER:
        assert np.abs(R.resize(R.flip_np(z, v), 23, 19) - R.flip_np(R.resize(z, 23, 19), v)).max() < 1e-12
    a, bs = z.astype(np.float32), {v: rng.normal(0.0, 3.0, z.shape).astype(np.float32) for v in R.ORDER}
    d64 = R.margin_f64(a, bs, 23, 19)
    merged = (a.astype(np.float64) + sum(R.flip_np(b.astype(np.float64), v) for v, b in bs.items())) / 4.0
    low = R.resize(merged, 23, 19)
    assert np.abs((low[..., 1] - low[..., 0]) - d64).max() < 1e-12
    assert np.abs(R.margin_f32(a, bs, 23, 19) - d64).max() <= R.tau_of(a, *bs.values()) / 4
