"""Host half of device-side scoring (no GPU): metrics.iou_from_counts against metrics.iou, the `--device-metrics` flag down to the
meta-learner's keyword, and Gecko's scoring helper driven by a stub learner whose score_resident returns prepared counts."""
import contextlib
import io

import numpy as np
import pytest
import torch

from mliis_amd import args as A
from mliis_amd import metrics
from mliis_amd.reptile import FOMLIS, Gecko, SingleRank


def _counts(p, l):
    return [int(np.count_nonzero(p & l)), int(np.count_nonzero(p | l)), int(np.count_nonzero(p)), int(np.count_nonzero(l))]


def test_iou_from_counts_is_metrics_iou():
    rng = np.random.default_rng(0)
    for k in range(40):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        p = rng.random((h, w)) < rng.random()
        l = rng.random((h, w)) < rng.random()
        if k == 0:
            p[:], l[:] = False, False            # empty mask against an empty label: (0 + eps) / (0 + eps)
        pred = np.stack([~p, p], axis=-1).astype(np.float32)
        lab = np.stack([~l, l], axis=-1).astype(np.float32)
        c = _counts(p, l)
        assert metrics.iou_from_counts(c[0], c[1]) == metrics.iou(pred, lab)
        assert metrics.iou_from_counts(np.int32(c[0]), np.int64(c[1])) == metrics.iou(pred, lab)
    assert metrics.iou_from_counts(0, 0) == 1.0
    assert metrics.iou_from_counts(4, 12) == (4 + 1e-7) / (12 + 1e-7)          # SURVEY Appendix F's golden case
    assert metrics.iou_from_counts(4, 12, epsilon=0.5) == 4.5 / 12.5
    assert isinstance(metrics.iou_from_counts(np.int32(3), np.int32(5)), float)


def test_flag_parses_and_reaches_the_meta_learner():
    a = A.argument_parser().parse_args(["--device-metrics"])
    assert a.device_metrics is True
    assert A.argument_parser().parse_args([]).device_metrics is False
    assert A.evaluate_kwargs(a)["device_metrics"] is True and A.train_kwargs(a)["device_metrics"] is True
    off = A.argument_parser().parse_args([])
    assert A.evaluate_kwargs(off)["device_metrics"] is False and A.train_kwargs(off)["device_metrics"] is False
    # the reference's parser does not know the flag
    ref = A.argument_parser(extensions=False)
    assert not hasattr(ref.parse_args([]), "device_metrics")
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        ref.parse_args(["--device-metrics"])
    assert A.evaluate_kwargs(ref.parse_args([]))["device_metrics"] is False
    # ... and the drivers hand it to the meta-learner as its keyword -- only when set
    from mliis_amd import eval as E
    from mliis_amd import train as T
    seen = []

    class Meta:
        dist = SingleRank()

        def __init__(self, learner, **kw):
            seen.append(kw)

        def evaluate(self, dataset, **kw):
            return 0.5, {"t": 0.5}

        def train_step(self, *a, **kw):
            pass

        def evaluate_m_k_shot_ranges_all_tasks(self, **kw):
            return [1], [0.5]

    with contextlib.redirect_stdout(io.StringIO()):
        for dm in (True, False):
            E.evaluate_gecko(object(), [], num_samples=1, meta_fn=Meta, device_metrics=dm)
            E.run_k_shot_learning_curves_experiment(object(), [], num_samples=1, meta_fn=Meta, csv_outpath=None, device_metrics=dm)
    assert [kw.get("device_metrics") for kw in seen] == [True, True, None, None]
    del seen[:]

    class Lrn:
        def synchronize(self):
            pass

        def named_numpy(self):
            return {"w": np.zeros(1, np.float32)}

    import tempfile
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(io.StringIO()):
        for dm in (True, False):
            T.train_gecko(Lrn(), [], [], d, meta_iters=1, eval_interval=0, meta_fn=Meta, verbose=False, device_metrics=dm)
    assert [kw.get("device_metrics") for kw in seen] == [True, None]


class _Stub:
    """The learner protocol as far as Gecko._evaluate uses it; score_resident hands out prepared counts and records its batches."""
    n_trainable = 1

    def __init__(self, rows_of):
        self.rows_of, self.calls, self.steps = rows_of, [], []

    def export_all(self):
        return {}

    def import_all(self, st):
        pass

    def load_task(self, x, y):
        pass

    def inner_step(self, idx, **kw):
        self.steps.append(list(idx))

    def score_resident(self, idx, training=False):
        assert training is False
        self.calls.append(list(idx))
        return np.asarray([self.rows_of[i] for i in idx], dtype=np.int64)


class _NoScore(_Stub):
    score_resident = None


def test_gecko_needs_a_scoring_learner():
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="score_resident"):
            Gecko(_NoScore({}), device_metrics=True, dist=SingleRank())
        with pytest.raises(ValueError, match="score_resident"):
            Gecko(_Stub({}), lanes=[_NoScore({})], device_metrics=True, dist=SingleRank())
        with pytest.raises(ValueError, match="score_resident"):
            FOMLIS(_NoScore({}), device_metrics=True, dist=SingleRank())
        from oracle import efficientlab_ref as R
        with pytest.raises(ValueError, match="score_resident"):
            Gecko(R.OracleLearner(image_size=32, seed=0, dtype=torch.float64, lr=1e-3), device_metrics=True, dist=SingleRank())
        assert Gecko(_NoScore({}), dist=SingleRank()).device_metrics is False            # the default needs nothing new
        assert Gecko(_Stub({}), device_metrics=True, dist=SingleRank()).device_metrics is True


@pytest.mark.parametrize("transductive", [False, True])
def test_evaluate_scores_from_the_counts(transductive):
    # train images carry counts that would give IoU 0: the per-sample setting must keep the LAST row of each batch only
    rows = {i: [0, 50, 25, 25] for i in range(5)}
    rows.update({5: [4, 12, 8, 8], 6: [0, 0, 0, 0], 7: [3, 9, 5, 7]})
    L = _Stub(rows)
    train_idx, test_idx = [0, 1, 2, 3, 4], [5, 6, 7]
    with contextlib.redirect_stdout(io.StringIO()):
        g = Gecko(L, transductive=transductive, device_metrics=True, rng_mode="reference", dist=SingleRank())
        got = g._evaluate(train_idx, test_idx, labels=None, inner_batch_size=4, inner_iters=2, replacement=False)
        es = g._early_stopping_learn(train_idx, test_idx, None, 4, min_steps=1, max_steps=2, replacement=False, lr=1e-3)
    want = float(np.nanmean([(4 + 1e-7) / (12 + 1e-7), 1.0, (3 + 1e-7) / (9 + 1e-7)]))
    assert got == want and es == (1, want)
    one = [test_idx] if transductive else [train_idx + [t] for t in test_idx]
    assert L.calls == one * 3 and len(L.steps) == 4               # one scoring round per _evaluate, one per early-stopping step


def test_score_library_exports_its_header_and_nothing_else():
    """libmliis_score.so (csrc/score.hip) against include/mliis_score.h: its dynamic symbols are the header's declarations, the ctypes
    table has their argument counts, none of them belongs to the training library's C ABI, and the code object holds no packed fp32
    instruction with op_sel:[0,1] (csrc/common.hpp, lone())."""
    import os
    import re
    import subprocess
    import sys
    from mliis_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(_lib.SCORE_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mliis_score.h")).read(), flags=re.S)
    decls = {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
             for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.SCORE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(decls) == set(_lib.SCORE_SIGNATURES) == syms
    for name, params in decls.items():
        assert len(params) == len(_lib.SCORE_SIGNATURES[name][1]), name
    assert not set(decls) & set(_lib.SIGNATURES)
    sys.path.insert(0, os.path.join(root, "tools"))
    from check_packed_forms import affected_kernels
    assert affected_kernels(_lib.SCORE_LIB_PATH) == {}
    assert _lib.score_lib.load().mliis_score_last_error() == b""
