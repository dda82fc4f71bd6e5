"""The threshold sweep without a GPU: the host arithmetic of mliis_amd.metrics (counts / curves / reliability / summary from histograms)
against brute-force numpy, the flags, the meta-learner's sink driven by a stub learner, libmliis_sweep.so against its header (in tree and
from a clean out-of-tree build), and the whole program on the CPU oracle learner with a histogram computed on the host."""
import contextlib
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from mliis_amd import args as A
from mliis_amd import metrics as M
from mliis_amd.reptile import FOMLIS, Gecko, SingleRank
from test_build_cpu import _affected_packed_forms, _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_sweep_last_error", "mliis_prob_hist_bins", "mliis_prob_histogram"}
BINS = 256


# ------------------------------------------------------------------------------------------------ host arithmetic
def _bin(p):
    """The stated rule, on float32 probabilities: b = clamp(ceil(p * 256) - 1, 0, 255) (p * 256 is exact)."""
    p = np.asarray(p, dtype=np.float32)
    return np.clip(np.ceil(p * np.float32(256)).astype(np.int64) - 1, 0, BINS - 1)


def _histogram(p, lab):
    """int64 [n, 2, 256] from probabilities [n, m] and boolean labels [n, m]."""
    h = np.zeros((len(p), 2, BINS), dtype=np.int64)
    for n in range(len(p)):
        np.add.at(h[n], (np.asarray(lab[n], dtype=np.int64), _bin(p[n])), 1)
    return h


def _random_case(seed, n=4, m=3000):
    rng = np.random.default_rng(seed)
    p = rng.random((n, m)).astype(np.float32)
    p[:, :400] = np.float32(1) / (np.float32(1) + np.exp(rng.normal(0, 8, (n, 400)).astype(np.float32)))      # saturated: piles at both ends
    exact = [0.0, 1.0, 0.5, 1 / 256, 2 / 256, 127 / 256, 128 / 256, 129 / 256, 200 / 256, 255 / 256]
    p[:, 400:400 + len(exact)] = np.asarray(exact, dtype=np.float32)
    p[:, 420:440] = np.nextafter(np.float32(0.5), np.float32(1))                   # the smallest value above the threshold
    p[:, 440:460] = np.nextafter(np.float32(0.5), np.float32(0))
    lab = rng.random((n, m)) < 0.35
    lab[:, 400:400 + len(exact)] = rng.random((n, len(exact))) < 0.5
    return p, lab


@pytest.mark.parametrize("seed", [0, 1])
def test_counts_and_curves_equal_brute_force(seed):
    p, lab = _random_case(seed)
    h = _histogram(p, lab)
    counts, curve = M.counts_from_histogram(h), M.iou_curve(h)
    assert counts.dtype == np.int64 and counts.shape == (len(p), BINS, 4) and curve.dtype == np.float64 and curve.shape == (len(p), BINS)
    for n in range(len(p)):
        for k in range(BINS):
            P = (p[n] > np.float32(k / 256)) if k else np.ones_like(lab[n])       # row 0: everything predicted
            want = [int((P & lab[n]).sum()), int((P | lab[n]).sum()), int(P.sum()), int(lab[n].sum())]
            assert counts[n, k].tolist() == want, (n, k)
            assert curve[n, k] == M.iou_from_counts(want[0], want[1])
        # k = 128 is the project's rule: p > 0.5f; p == 0.5 exactly is not predicted
        pred = np.stack([1 - p[n], p[n]], axis=-1)[None].astype(np.float64)
        pred = (pred > 0.5).astype(np.float32)
        assert curve[n, 128] == M.iou(pred[0][None], np.stack([~lab[n], lab[n]], axis=-1).astype(np.float32)[None])
    assert np.array_equal(M.counts_from_histogram(h.astype(np.int32)), counts)            # the device's words
    assert np.array_equal(M.counts_from_histogram(h[0]), counts[0])                       # any leading shape
    assert _bin([0.0, 1.0, 0.5, 129 / 256]).tolist() == [0, 255, 127, 128]
    for bad in (np.zeros((2, 255)), np.zeros((3, 256), dtype=np.int64), np.zeros((2, 256), dtype=np.float32)):
        with pytest.raises(ValueError):
            M.counts_from_histogram(bad)


def test_empty_labels_and_empty_predictions_take_the_epsilon_form():
    h = np.zeros((3, 2, BINS), dtype=np.int64)
    h[0, 0, 3] = 500                  # no label pixel, every probability below 4/256
    h[1, 1, 250] = 40                 # labelled pixels only, all confident
    h[1, 0, 0] = 60
    # image 2: no pixels at all
    curve, counts = M.iou_curve(h), M.counts_from_histogram(h)
    assert counts[0, 128].tolist() == [0, 0, 0, 0] and curve[0, 128] == 1.0 == M.iou_from_counts(0, 0)      # nothing predicted, nothing labelled
    assert counts[0, 2].tolist() == [0, 500, 500, 0] and curve[0, 2] == (0 + 1e-7) / (500 + 1e-7)
    assert counts[1, 251].tolist() == [0, 40, 0, 40] and curve[1, 251] == (0 + 1e-7) / (40 + 1e-7)          # an empty prediction
    assert counts[1, 250].tolist() == [40, 40, 40, 40] and curve[1, 250] == 1.0
    assert counts[1, 0].tolist() == [40, 100, 100, 40]
    assert np.all(curve[2] == 1.0)


def test_reliability_table_and_ece():
    h = np.zeros((2, 2, BINS), dtype=np.int64)
    h[0, 0, 0], h[0, 1, 0] = 90, 10           # bin 0 (confidence 0.5/256): 10 % foreground
    h[1, 1, 255], h[1, 0, 255] = 30, 10       # bin 255 (confidence 255.5/256): 75 % foreground
    h[1, 1, 127] = 60                         # bin 127: all foreground
    r = M.reliability(h)
    assert r["pixels"] == 200 and r["count"][0] == 100 and r["count"][255] == 40 and r["count"][127] == 60 and sum(r["count"]) == 200
    assert r["foreground_share"][0] == 0.1 and r["foreground_share"][255] == 0.75 and r["foreground_share"][127] == 1.0
    assert r["foreground_share"][5] is None and r["confidence"][0] == 0.5 / 256 and r["confidence"][255] == 255.5 / 256
    want = (100 * abs(0.1 - 0.5 / 256) + 40 * abs(0.75 - 255.5 / 256) + 60 * abs(1.0 - 127.5 / 256)) / 200
    assert r["ece"] == pytest.approx(want, rel=1e-12)
    json.dumps(r)
    assert np.isnan(M.reliability(np.zeros((2, BINS), dtype=np.int64))["ece"])


def test_threshold_summary_and_its_tie_rule():
    flat = np.full((2, BINS), 0.25)
    s = M.threshold_summary(flat)
    assert s["thresholds"] == [k / 256 for k in range(1, 256)] and len(s["mean_iou"]) == 255
    assert s["best_threshold"] == 0.5 and s["iou_at_best"] == s["iou_at_0.5"] == 0.25              # all equal: the one at 0.5
    c = flat.copy()
    c[:, [100, 140, 200]] = 0.5
    assert M.best_threshold_index(c.mean(axis=0)) == 140 and M.threshold_summary(c)["best_threshold"] == 140 / 256      # |140 - 128| < |100 - 128|
    c[:, 116] = 0.5
    assert M.best_threshold_index(c.mean(axis=0)) == 116                                            # equally near: the smaller
    c[:, 0] = 9.0
    assert M.best_threshold_index(c.mean(axis=0)) == 116                                            # row 0 is no threshold
    c[:, 30] = 0.75
    s = M.threshold_summary(c)
    assert s["best_threshold"] == 30 / 256 and s["iou_at_best"] == 0.75 and s["iou_at_0.5"] == 0.25
    # the mean at 0.5 is the evaluation loops' own, float(np.nanmean(list)); NaN rows are left out of every threshold's mean
    rng = np.random.default_rng(3)
    curves = rng.random((11, BINS))
    curves[4] = np.nan
    m = M.mean_curve(curves)
    assert m[128] == float(np.nanmean([row[128] for row in curves]))                               # to the last bit
    assert np.allclose(m, [float(np.nanmean([row[k] for row in curves])) for k in range(BINS)], rtol=1e-14, atol=0)
    assert M.threshold_summary(curves)["iou_at_0.5"] == float(np.nanmean(list(curves[:, 128])))


def test_sink_aggregates_as_the_printed_mean_does():
    rng = np.random.default_rng(5)
    sink, passes = M.ThresholdSweep(), []
    for i in range(3):
        sink.begin_pass(i)
        tasks = []
        for name in ("a", "b", "c")[:2 + i % 2]:
            h = rng.integers(0, 50, (4, 2, BINS))
            sink(name, M.iou_curve(h), h)
            tasks.append(float(np.nanmean([float(v) for v in M.iou_curve(h)[:, 128]])))       # Gecko._evaluate: the task's class_iou
        passes.append(float(np.nanmean(tasks)))                                                # Gecko.evaluate: the pass's mean
    doc = sink.summary()
    assert doc["iou_at_0.5"] == float(np.nanmean(passes))                                      # evaluate_gecko: the mean of samples
    assert set(doc["tasks"]) == {"a", "b", "c"} and doc["reliability"]["pixels"] == int(sink.pooled.sum()) > 0
    json.dumps(doc)


# ------------------------------------------------------------------------------------------------ flags
def test_flags_parse_refuse_and_leave_the_keyword_tables_alone():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.threshold_sweep is False and off.threshold_sweep_val is False and A.threshold_sweep(off) == (False, False)
    on = p.parse_args(["--threshold-sweep"])
    assert A.threshold_sweep(on) == (True, False)
    val = p.parse_args(["--threshold-sweep-val", "--num_val_tasks", "3"])
    assert A.threshold_sweep(val) == (True, True)                                              # implies the sweep
    with pytest.raises(ValueError, match="num_val_tasks"):
        A.threshold_sweep(p.parse_args(["--threshold-sweep", "--threshold-sweep-val"]))
    with pytest.raises(ValueError, match="eval_val_tasks"):
        A.threshold_sweep(p.parse_args(["--threshold-sweep-val", "--num_val_tasks", "3", "--eval_val_tasks"]))
    assert A.threshold_sweep(p.parse_args(["--threshold-sweep", "--eval_val_tasks", "--num_val_tasks", "3"])) == (True, False)
    for a in (on, val):      # only the final pass is swept: nothing reaches the keyword tables of the other drivers
        b = p.parse_args(["--num_val_tasks", str(a.num_val_tasks)])
        assert A.evaluate_kwargs(a) == A.evaluate_kwargs(b) and "threshold_sweep" not in A.evaluate_kwargs(a)
        ta, tb = A.train_kwargs(a), A.train_kwargs(b)
        assert {k: v for k, v in ta.items() if k != "meta_fn"} == {k: v for k, v in tb.items() if k != "meta_fn"} and ta["meta_fn"] is tb["meta_fn"]
        assert A.model_kwargs(a) == A.model_kwargs(b)
    ref = A.argument_parser(extensions=False)
    assert not hasattr(ref.parse_args([]), "threshold_sweep") and A.threshold_sweep(ref.parse_args([])) == (False, False)
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        ref.parse_args(["--threshold-sweep"])


def test_main_refuses_a_val_sweep_without_val_tasks_before_building_anything():
    import run_metasegnet

    def no_learner(**kw):
        raise AssertionError("the learner was built")
    with pytest.raises(ValueError, match="num_val_tasks"), contextlib.redirect_stdout(io.StringIO()):
        run_metasegnet.main(["--image_size", "32", "--synthetic-tasks", "4", "--threshold-sweep-val"], learner_factory=no_learner, device="cpu")


def test_the_driver_passes_the_sink_only_when_set():
    from mliis_amd import eval as E
    seen = []

    class Meta:
        dist = SingleRank()

        def __init__(self, learner, **kw):
            seen.append(kw)

        def evaluate(self, dataset, **kw):
            return 0.5, {"t": 0.5}

    sink = M.ThresholdSweep()
    with contextlib.redirect_stdout(io.StringIO()):
        E.evaluate_gecko(object(), [], num_samples=3, meta_fn=Meta, threshold_sweep=sink)
        E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta)
    assert seen[0]["threshold_sweep"] is sink and "threshold_sweep" not in seen[1] and len(sink.passes) == 3


# ------------------------------------------------------------------------------------------------ the meta-learner's sink
class _Stub:
    """The learner protocol as far as Gecko._evaluate uses it; histogram_resident hands out prepared histograms and records its calls."""
    n_trainable = 1

    def __init__(self, hist_of, H=4):
        self.hist_of, self.calls, self.H = hist_of, [], H

    def export_all(self):
        return {}

    def import_all(self, st):
        pass

    def load_task(self, x, y):
        pass

    def inner_step(self, idx, **kw):
        pass

    def score_resident(self, idx, training=False):
        raise AssertionError("the sweep replaces the counts call")

    def mask_resident(self, idx, **kw):
        raise AssertionError("the sweep's call returns the masks")

    def histogram_resident(self, idx, training=False, last_only=False, masks=False):
        assert training is False
        self.calls.append((list(idx), last_only, masks))
        h = np.asarray([self.hist_of[i] for i in (idx[-1:] if last_only else idx)], dtype=np.int64)
        return (h, np.zeros((len(h), self.H, self.H), dtype=bool)) if masks else h


class _NoHist(_Stub):
    histogram_resident = None


class _Writer:
    overlays = False

    def __init__(self):
        self.saved = []

    def save(self, task, sample, j, mask, image=None):
        self.saved.append((task, sample, j, mask.shape))


@pytest.mark.parametrize("transductive", [False, True])
def test_evaluate_scores_from_the_histograms_and_feeds_the_sink(transductive):
    rng = np.random.default_rng(7)
    hist_of = {i: rng.integers(0, 9, (2, BINS)) for i in range(8)}
    train_idx, test_idx = [0, 1, 2, 3, 4], [5, 6, 7]
    want = float(np.nanmean([float(M.iou_curve(hist_of[t])[128]) for t in test_idx]))
    for writer in (None, _Writer()):
        L, got = _Stub(hist_of), []
        sink = lambda *a: got.append(a)   # noqa: E731
        with contextlib.redirect_stdout(io.StringIO()):
            g = Gecko(L, transductive=transductive, device_metrics=True, rng_mode="reference", dist=SingleRank(), threshold_sweep=sink,
                      **({"prediction_writer": writer} if writer else {}))
            iou = g._evaluate(train_idx, test_idx, labels=None, inner_batch_size=4, inner_iters=2, replacement=False, task_name="t",
                              eval_sample_num=1)
        assert iou == want
        m = writer is not None
        assert L.calls == ([(test_idx, False, m)] if transductive else [(train_idx + [t], True, m) for t in test_idx])
        (name, curves, hists), = got
        assert name == "t" and curves.shape == (3, BINS) and np.array_equal(hists, [hist_of[t] for t in test_idx])
        assert np.array_equal(curves, M.iou_curve(hists))
        if writer:
            assert writer.saved == [("t", 1, j, (4, 4)) for j in range(3)]
    with contextlib.redirect_stdout(io.StringIO()):
        for cls in (Gecko, FOMLIS):
            with pytest.raises(ValueError, match="histogram_resident"):
                cls(_NoHist({}), dist=SingleRank(), threshold_sweep=M.ThresholdSweep())
        with pytest.raises(ValueError, match="histogram_resident"):
            Gecko(_Stub({}), lanes=[_NoHist({})], dist=SingleRank(), threshold_sweep=M.ThresholdSweep())
        assert Gecko(_NoHist({}), dist=SingleRank()).threshold_sweep is None                   # the default needs nothing new


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_sweep.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_sweep_library(tmp_path):
    """A clean out-of-tree `make BUILD=... all` links the library: one translation unit, the shared export map, exactly the header's names
    as dynamic symbols, a gfx950 code object only and none of the packed fp32 forms test_build_cpu keeps out of the step's library; the
    in-tree libraries are not disturbed."""
    build = str(tmp_path / "obj")
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    intree = os.path.join(ROOT, "mliis_amd", "libmliis_sweep.so")
    before = os.path.getmtime(intree) if os.path.exists(intree) else None
    r = subprocess.run(["make", "-C", CSRC, "-j" + jobs, "BUILD=" + build, "all"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    so = os.path.join(build, "libmliis_sweep.so")
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "sweep.o"))
    line = next(ln for ln in r.stdout.splitlines() if " sweep.hip " in ln + " ")
    assert "-fno-slp-vectorize" in line and "--offload-arch=gfx950" in line
    assert any("--version-script=exports.map" in ln and "libmliis_sweep.so" in ln for ln in r.stdout.splitlines())
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    assert (os.path.getmtime(intree) if os.path.exists(intree) else None) == before
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(SWEEP_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(SWEEP_OBJS\) \$\(SWEEP_TARGET\)", mk)


def test_sweep_library_exports_its_header_and_refuses_bad_arguments_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.SWEEP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.SWEEP_SIGNATURES) == set(_dynamic_symbols(_lib.SWEEP_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.SWEEP_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES) |
                             set(_lib.LAYERLOG_SIGNATURES) | set(_lib.CLIP_SIGNATURES))
    assert _affected_packed_forms(_lib.SWEEP_LIB_PATH) == {}
    lib = _lib.sweep_lib
    assert lib.load().mliis_sweep_last_error() == b"" and lib.size("mliis_prob_hist_bins") == BINS == M.HIST_BINS
    # the entry point refuses what it can without touching a device: nothing is launched for a null pointer or a bad shape
    raw = lib.load().mliis_prob_histogram
    assert raw(None, None, None, 1, 4, 4, 8, 8, None, None) == -1 and lib.load().mliis_sweep_last_error().startswith(b"prob_histogram: null")
    assert raw(8, 8, None, 0, 4, 4, 8, 8, 8, None) == -1 and raw(8, 8, None, 65536, 4, 4, 8, 8, 8, None) == -1
    assert raw(8, 8, None, 1, 9, 4, 8, 8, 8, None) == -1 and b"smaller" in lib.load().mliis_sweep_last_error()
    assert raw(8, 8, None, 1, 4, 4, 46341, 46341, 8, None) == -2                       # past 32-bit pixel counts
    assert raw(12, 8, None, 1, 4, 4, 8, 8, 8, None) == -3 and raw(8, 8, None, 1, 4, 4, 8, 8, 10, None) == -3


def test_build_entry_loads_the_library_lazily_in_the_package():
    """build() loads the new library; importing the package and its ops does not."""
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "sweep_lib.load()" in src
    code = "import mliis_amd, mliis_amd.ops, mliis_amd.learner, mliis_amd.reptile, mliis_amd._lib as L; assert L.sweep_lib._dll is None; print('ok')"
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the whole program on the CPU oracle
H = 32


def _factory(device=None, feature_extractor_name="efficientnet-b0", image_size=H, rsd=(2, 4), learning_rate=1e-3, l2=False, dice=False,
             label_smoothing=0.0, seed=0, **_ignored):
    from oracle import efficientlab_ref as R

    class SweepingOracle(R.OracleLearner):
        """The oracle learner with the histogram computed on the host: float32 softmax of its full-resolution logits, the stated bin rule."""

        def histogram_resident(self, idx, training=False, last_only=False, masks=False):
            idx = list(idx)
            with torch.no_grad():
                logits, _ = R.forward(self.a, self.params, self.bn, self._x[idx], training, round_ops=self.round_ops)
            p1 = torch.softmax(logits.float(), dim=-1)[..., 1].numpy().reshape(len(idx), -1)
            lab = (np.rint(self._y[idx].numpy()[..., 1]) != 0).reshape(len(idx), -1)
            h = _histogram(p1, lab)
            n0 = len(idx) - 1 if last_only else 0
            return (h[n0:], (p1 > 0.5).reshape(len(idx), self.a.image_size, self.a.image_size)[n0:]) if masks else h[n0:]

    torch.set_num_threads(4)
    return SweepingOracle(name=feature_extractor_name, image_size=image_size, rsd=tuple(rsd or ()), seed=seed, dtype=torch.float32,
                          lr=learning_rate, l2=l2, dice=dice, label_smoothing=label_smoothing, drop_connect=False)


def test_main_writes_the_sweep_file_and_its_iou_at_half_is_the_printed_mean(tmp_path):
    import run_metasegnet
    base = ["--image_size", str(H), "--rsd", "2", "4", "--sgd", "--shots", "2", "--inner-batch", "2", "--inner-iters", "2", "--meta-batch", "2",
            "--eval-samples", "2", "--eval-iters", "1", "--eval-batch", "2", "--synthetic-tasks", "6", "--meta-step", "0.5",
            "--learning-rate", "0.01", "--skip-train-task-eval", "--meta-iters", "1", "--eval-interval", "0", "--num_val_tasks", "2"]
    d = str(tmp_path / "ckpt")
    outs = []
    for extra in ([], ["--pretrained", "--threshold-sweep"], ["--pretrained", "--threshold-sweep-val"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            run_metasegnet.main(base + ["--checkpoint", d] + extra, learner_factory=_factory, device="cpu")
        outs.append(buf.getvalue())
        path = os.path.join(d, "meta-test_threshold_sweep.json")
        if not extra:
            assert not os.path.exists(path)                                            # nothing new without the flag
            continue
        doc = json.load(open(path))
        printed = float(next(ln for ln in outs[-1].splitlines() if ln.startswith("Mean IoU over all meta-test tasks: ")).split(": ")[1])
        assert doc["iou_at_0.5"] == printed == doc["mean_iou"][127]
        assert doc["thresholds"] == [k / 256 for k in range(1, 256)] and doc["iou_at_best"] >= doc["iou_at_0.5"]
        assert doc["best_threshold"] == M.best_threshold_index([np.nan] + doc["mean_iou"]) / 256
        assert set(doc["tasks"]) == set(json.load(open(os.path.join(d, "meta-test_results.json"))))
        assert sum(doc["reliability"]["count"]) == doc["reliability"]["pixels"] == 2 * 5 * H * H      # passes x test shots x pixels
        assert ("selected_on_val" in doc) == (extra[-1] == "--threshold-sweep-val")
        if "selected_on_val" in doc:
            sel = doc["selected_on_val"]
            k = M.best_threshold_index([np.nan] + sel["val_mean_iou"])
            assert sel["threshold"] == k / 256 and sel["val_iou"] == sel["val_mean_iou"][k - 1] and sel["test_iou_at_threshold"] == doc["mean_iou"][k - 1]
    strip = lambda o: [ln for ln in o.splitlines() if not ln.startswith("Experiment ")]   # noqa: E731
    assert strip(outs[1]) == strip(outs[2])                                            # the val pass prints nothing
