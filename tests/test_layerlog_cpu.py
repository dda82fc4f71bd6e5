"""The inner loop's per-tensor log, the host half: the chunk table (mliis_amd/layerlog.py) and its validator, the record decoder, the
attribution of a non-finite step to tensors and the per-meta-iteration row on hand-made records, the flags, DivergenceError's optional
attributes, libmliis_layerlog.so's build and exported ABI against include/mliis_layerlog.h, and the meta-learners' use of the log on a
stub learner that wraps the CPU oracle and emits rows."""
import contextlib
import io
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from mliis_amd import args as A
from mliis_amd import layerlog as LL
from mliis_amd import metaseg, spec
from mliis_amd import steplog as S
from mliis_amd.reptile import FOMLIS, Gecko
from mliis_amd.train import train_gecko
from oracle import efficientlab_ref as R
from test_build_cpu import _affected_packed_forms, _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_layerlog_last_error", "mliis_layerlog_chunk_quads", "mliis_layerlog_workspace_bytes", "mliis_layerlog_record_words",
         "mliis_layerlog_append"}
CQ = 8   # a chunk of 8 quads = 32 floats: small enough to write the expected tables by hand


# ------------------------------------------------------------------------------------------------ the chunk table
def _check_table(sizes, cq):
    """The properties every table has: chunks tile every tensor's quads exactly once and in order, none crosses a tensor or exceeds the
    chunk size, valid elements sum to the sizes, chunk ranges are contiguous, tensors sit at the arena's padded offsets."""
    t = LL.chunk_table(sizes, cq)
    assert t.chunks.dtype == np.int32 and t.segs.dtype == np.int32 and t.chunks.shape[1] == 4 and t.segs.shape == (len(sizes), 4)
    assert t.n == sum((s + 3) // 4 * 4 for s in sizes)
    off, next_chunk = 0, 0
    for k, size in enumerate(sizes):
        q0, count, c0, c1 = t.segs[k].tolist()
        assert q0 * 4 == off and count == size and c0 == next_chunk and c1 > c0
        quads = (size + 3) // 4
        assert c1 - c0 == (quads + cq - 1) // cq
        at, valid = q0, 0
        for c in range(c0, c1):
            ct, cq0, cquads, cvalid = t.chunks[c].tolist()
            assert ct == k and cq0 == at and 1 <= cquads <= cq and (cquads == cq or c == c1 - 1)
            assert cvalid == (4 * cquads if c < c1 - 1 else size - 4 * (at - q0))
            at += cquads
            valid += cvalid
        assert at == q0 + quads and valid == size
        off += quads * 4
        next_chunk = c1
    assert next_chunk == len(t.chunks)
    LL.validate_table(t.chunks, t.segs, t.n, cq)
    return t


def test_chunk_table_on_small_size_lists():
    t = _check_table([7], CQ)
    assert t.chunks.tolist() == [[0, 0, 2, 7]] and t.segs.tolist() == [[0, 7, 0, 1]] and t.n == 8
    t = _check_table([1, 2, 3, 4, 5], CQ)
    assert t.chunks.tolist() == [[0, 0, 1, 1], [1, 1, 1, 2], [2, 2, 1, 3], [3, 3, 1, 4], [4, 4, 2, 5]] and t.n == 24
    # sizes straddling one chunk (32 floats) and three
    t = _check_table([31, 32, 33, 95, 96, 97], CQ)
    assert [int(c1 - c0) for _, _, c0, c1 in t.segs.tolist()] == [1, 1, 2, 3, 3, 4]
    assert t.chunks[3].tolist() == [2, 24, 1, 1]                 # the 33rd float of tensor 2: a chunk of one quad, one element valid
    assert t.chunks[-1].tolist() == [5, 16 + 9 + 24 + 24 + 24, 1, 1]
    for bad in ([], [0], [4, -1]):
        with pytest.raises(ValueError):
            LL.chunk_table(bad, CQ)
    with pytest.raises(ValueError):
        LL.chunk_table([4], 0)


@pytest.mark.parametrize("name,size,T", [("efficientnet-b0", 224, 169), ("efficientnet-b3", 384, 361)])
def test_chunk_table_of_the_real_arenas(name, size, T):
    arch = spec.derive(name, size, [2, 4], 0.0, False, skip_decoding=False)
    sizes = [p.size for p in spec.param_table(arch) if p.trainable]
    assert len(sizes) == T
    t = _check_table(sizes, 4096)
    assert len(t.chunks) >= T and len(t.chunks) <= T + t.n // (4 * 4096)


def test_every_kind_of_bad_table_is_refused():
    t = LL.chunk_table([5, 70, 3], CQ)      # tensors of 2, 18 (three chunks) and 1 quads
    LL.validate_table(t.chunks, t.segs, t.n, CQ)

    def bad(chunks=None, segs=None, n=None, cq=CQ, at=None, value=None, of="chunks"):
        c, s = t.chunks.copy() if chunks is None else chunks, t.segs.copy() if segs is None else segs
        if at is not None:
            (c if of == "chunks" else s)[at] = value
        with pytest.raises(ValueError):
            LL.validate_table(c, s, t.n if n is None else n, cq)

    bad(n=t.n - 4)                                   # the last tensor leaves the arena
    bad(n=t.n + 2)                                   # n no multiple of 4
    bad(n=0)
    bad(cq=4)                                        # chunks longer than the chunk size
    bad(chunks=t.chunks.astype(np.int64))            # wrong dtype
    bad(chunks=t.chunks[:, :3])                      # wrong shape
    bad(segs=t.segs.reshape(-1))
    bad(chunks=t.chunks[:0])                         # empty
    bad(of="segs", at=(1, 1), value=0)               # a tensor without elements
    bad(of="segs", at=(1, 0), value=1)               # overlaps the tensor before it (not ascending)
    bad(of="segs", at=(2, 0), value=t.n // 4)        # starts past the arena
    bad(of="segs", at=(1, 2), value=2)               # chunk range does not continue where the last one ended
    bad(of="segs", at=(2, 3), value=9)               # chunk range past the chunk table
    bad(of="segs", at=(1, 3), value=3)               # a tensor's chunks do not cover it
    bad(of="segs", at=(1, 1), value=90)              # count larger than what the chunks cover (and crosses into the next tensor)
    bad(at=(2, 0), value=0)                          # a chunk of another tensor in the range
    bad(at=(2, 1), value=11)                         # chunks not in order / with a gap
    bad(at=(1, 2), value=9)                          # a chunk crossing its share
    bad(at=(1, 2), value=0)                          # an empty chunk
    bad(at=(3, 3), value=8)                          # valid elements beyond the tensor's count (70 = 32 + 32 + 6)
    bad(at=(1, 3), value=31)                         # an inner chunk that is not wholly valid
    bad(at=(0, 3), value=8)                          # padding counted as valid
    bad(chunks=np.concatenate([t.chunks, t.chunks[-1:]]))   # a chunk that belongs to no tensor
    misaligned = t.segs.copy()                       # (first QUAD: alignment to 4 floats is in the unit; a gap between tensors is allowed)
    misaligned[2, 0] += 1
    moved = t.chunks.copy()
    moved[4, 1] += 1
    LL.validate_table(moved, misaligned, t.n + 4, CQ)


# ------------------------------------------------------------------------------------------------ decode / attribute / summarise
def _rows(values):
    """[steps, T] records from nested tuples."""
    r = np.zeros((len(values), len(values[0])), dtype=LL.RECORD_DTYPE)
    for k, row in enumerate(values):
        for t, rec in enumerate(row):
            r[k, t] = rec
    return r


def _steps(rows):
    r = np.zeros(len(rows), dtype=S.RECORD_DTYPE)
    for k, row in enumerate(rows):
        r[k] = row
    return r


N = LL.NONE
OK = lambda g, a, w=2.0: (g, a, w, 1.0, 0, 0, N, N)   # noqa: E731


def test_decode_orders_rows_across_the_wrap():
    ring = np.zeros((4, 3, 8), dtype=np.int32)
    rec = ring.view(LL.RECORD_DTYPE).reshape(4, 3)
    for k in range(6):
        rec[k % 4] = [(float(10 * k + t), 0, 0, 0, 0, 0, N, N) for t in range(3)]
    r, dropped = LL.decode(ring, 6, 3)
    assert r.shape == (3, 3) and r["x_l2"][:, 0].tolist() == [30.0, 40.0, 50.0] and r["x_l2"][2].tolist() == [50.0, 51.0, 52.0] and dropped == 0
    r, dropped = LL.decode(ring, 6, 0)
    assert r["x_l2"][:, 1].tolist() == [21.0, 31.0, 41.0, 51.0] and dropped == 2
    r, dropped = LL.decode(ring, 6, 6)
    assert r.shape == (0, 3) and dropped == 0
    assert int(r.dtype["x_first"].itemsize) == 4 and int(rec["x_first"][0, 0]) == 0xFFFFFFFF       # int32 -1 words read as "none"
    two = LL.split_tasks(LL.decode(ring, 6, 2)[0], 2, 2)
    assert [t["x_l2"][:, 0].tolist() for t in two] == [[20.0, 30.0], [40.0, 50.0]]
    for kw in (dict(steps_per_task=3, n_tasks=1), dict(steps_per_task=2, n_tasks=2, dropped=1), dict(steps_per_task=0, n_tasks=4)):
        with pytest.raises(ValueError):
            LL.split_tasks(r, **kw)
    with pytest.raises(ValueError):
        LL.decode(np.zeros((4, 8), dtype=np.int32), 1, 0)


def test_attribute_names_the_tensors_of_the_first_bad_step():
    names = ["t%d" % i for i in range(10)]
    clean = (1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0)
    # step 0 and 1 finite; at step 2 nine tensors have a non-finite gradient (a backward-born NaN upstream of tensor 9), one a parameter
    lay = _rows([[OK(1.0, float(t)) for t in range(10)],
                 [OK(1.0, a) for a in (5.0, 1.0, 9.0, 2.0, 9.0, 0.0, 7.0, 3.0, 8.0, 4.0)],
                 [(1.0, 1.0, 1.0, 1.0, 3 if t < 9 else 0, 1 if t == 4 else 0, 0 if t < 9 else N, 2 if t == 4 else N) for t in range(10)],
                 [OK(1.0, 1.0) for _ in range(10)]])
    st = _steps([clean, clean, (1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 27, 1), clean])
    found = LL.attribute(names, st, lay)
    assert found["step"] == 2 and found["grad_nonfinite"] == (9, names[:8]) and found["theta_nonfinite"] == (1, ["t4"])
    assert found["largest_grads"] == [("t2", 9.0), ("t4", 9.0), ("t8", 8.0)]     # ties in arena order
    # a NaN loss alone (the step log's view) with clean tensors: the step is still named, the lists are empty
    st1 = _steps([clean, (float("nan"), 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0)])
    found = LL.attribute(names, st1, lay[:2])
    assert found["step"] == 1 and found["grad_nonfinite"] == (0, []) and found["largest_grads"][0] == ("t9", 9.0)
    # a bad step 0: there is no finite step before it
    found = LL.attribute(names, st[2:], lay[2:])
    assert found["step"] == 0 and found["largest_grads"] is None and found["grad_nonfinite"][0] == 9
    assert LL.attribute(names, st[:2], lay[:2]) is None
    with pytest.raises(ValueError):
        LL.attribute(names[:9], st, lay)
    # DivergenceError: the positional form formats as it always did, the new attributes are optional keywords
    e = S.DivergenceError(1, 2, 3)
    assert str(e) == "inner loop diverged in meta-iteration 1: non-finite loss, gradient or parameters at task 2 step 3 of rank 0"
    assert (e.grad_nonfinite, e.theta_nonfinite, e.largest_grads) == (None, None, None) and e.rank == 0
    assert "another rank" in str(S.DivergenceError(3, None, None, rank=1)) and S.DivergenceError(3, 1, 1, 5).rank == 5
    found = LL.attribute(names, st, lay)
    e = S.DivergenceError(1, 2, 2, 0, grad_nonfinite=found["grad_nonfinite"], theta_nonfinite=found["theta_nonfinite"],
                          largest_grads=found["largest_grads"])
    assert str(e).startswith(str(S.DivergenceError(1, 2, 2))) and "gradient non-finite in 9 tensors: t0, t1" in str(e) and "t8 8" in str(e)
    assert e.theta_nonfinite == (1, ["t4"]) and e.largest_grads[0] == ("t2", 9.0)


def test_summary_row_with_a_zero_weight_norm_and_a_nan_row():
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    st = lambda lr: _steps([(1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0), (1.0, 1.0, 0.5, lr, 1.0, 1.0, 0, 0)])   # noqa: E731
    # two tasks of two steps over three tensors; tensor 1's parameters are all zero in task 5, tensor 2's gradient norm is NaN in task 3
    lay5 = _rows([[OK(8.0, 1.0), OK(2.0, 0.5), OK(1.0, 7.0)], [OK(4.0, 3.0, w=2.0), OK(1.0, 0.25, w=0.0), OK(3.0, 1.0, w=4.0)]])
    lay3 = _rows([[OK(6.0, 2.0), OK(4.0, 0.5), OK(3.0, 1.0)], [OK(2.0, 1.0, w=4.0), OK(3.0, 0.5, w=2.0), OK(float("nan"), 2.0, w=8.0)]])
    d5 = _rows([[(0.5, 0.1, 2.0, 1.0, 0, 0, N, N), (0.25, 0.1, 0.0, 0.0, 0, 0, N, N), (1.0, 0.1, 4.0, 1.0, 0, 0, N, N)]])[0]
    d3 = _rows([[(1.5, 0.1, 2.0, 1.0, 0, 0, N, N), (0.75, 0.1, 0.0, 0.0, 0, 0, N, N), (3.0, 0.1, 4.0, 1.0, 0, 0, N, N)]])[0]
    row = LL.summarize([(5, st(0.5), lay5, d5), (3, st(0.25), lay3, d3)], meta_iter=7)
    assert row["meta_iter"] == 7 and row["tasks"] == 2
    assert row["grad_l2_first"] == [7.0, 3.0, 2.0] and row["grad_l2_last"][:2] == [3.0, 2.0] and np.isnan(row["grad_l2_last"][2])
    # lr * grad_l2 / theta_l2 at the last step: (0.5 * 4 / 2 + 0.25 * 2 / 4) / 2; a zero theta_l2 in one task: None; NaN stays NaN
    assert row["grad_to_weight_last"][0] == (f32(0.5) * 4.0 / 2.0 + f32(0.25) * 2.0 / 4.0) / 2 and row["grad_to_weight_last"][1] is None
    assert np.isnan(row["grad_to_weight_last"][2])
    assert row["grad_absmax"] == [3.0, 0.5, 7.0]                              # over tasks and steps
    assert row["delta_l2"] == [1.0, 0.5, 2.0] and row["delta_rel"] == [0.5, None, 0.5]
    line = json.dumps({k: LL._json_value(v) for k, v in row.items()})
    assert "NaN" not in line and json.loads(line)["grad_l2_last"] == [3.0, 2.0, "nan"] and json.loads(line)["delta_rel"][1] is None
    empty = LL.summarize([], meta_iter=1)
    assert empty["tasks"] == 0 and empty["grad_l2_first"] is None


def test_writer_appends_rows_and_writes_the_names_once(tmp_path):
    d = str(tmp_path / "train")
    w = LL.LayerLogWriter(d, ["a", "b"])
    w.add({"meta_iter": 0, "grad_l2_last": [1.0, float("inf")], "first_nonfinite": None})
    w.add({"meta_iter": 2, "grad_l2_last": [1.0, 2.0], "first_nonfinite": {"task": 1, "step": 0}})
    assert json.load(open(os.path.join(d, "inner_loop_layers.names.json"))) == ["a", "b"]
    rows = [json.loads(ln) for ln in open(os.path.join(d, "inner_loop_layers.jsonl"))]
    assert [r["meta_iter"] for r in rows] == [0, 2] and rows[0]["grad_l2_last"] == [1.0, "inf"] and rows[1]["first_nonfinite"]["task"] == 1


# ------------------------------------------------------------------------------------------------ flags
def test_layer_log_flag_implies_the_step_log_and_is_absent_by_default():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.inner_loop_layer_log is False and off.inner_loop_layer_log_interval == 100 and not A.inner_loop_layer_log(off)
    assert not A.inner_loop_log(off) and "layer_log" not in A.model_kwargs(off) and "step_log" not in A.model_kwargs(off)
    assert not any(k.startswith("inner_loop_layer") for k in A.train_kwargs(off))
    plain = p.parse_args(["--inner-loop-log"])
    assert "layer_log" not in A.model_kwargs(plain) and not any(k.startswith("inner_loop_layer") for k in A.train_kwargs(plain))
    on = p.parse_args(["--inner-loop-layer-log", "--inner-iters", "100"])
    assert A.inner_loop_log(on) and on.inner_loop_log is False
    assert A.model_kwargs(on)["layer_log"] is True and A.model_kwargs(on)["step_log"] == 128
    tk = A.train_kwargs(on)
    assert tk["inner_loop_log"] is True and tk["on_divergence"] == "off" and tk["inner_loop_layer_log"] is True
    assert tk["inner_loop_layer_log_interval"] == 100
    assert A.train_kwargs(p.parse_args(["--inner-loop-layer-log", "--inner-loop-layer-log-interval", "7"]))["inner_loop_layer_log_interval"] == 7
    assert not any(k.startswith("inner_loop") for k in A.evaluate_kwargs(on))
    ref = A.argument_parser(extensions=False)
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        ref.parse_args(["--inner-loop-layer-log"])
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--inner-loop-layer-log" in readme and "--inner-loop-layer-log-interval" in readme


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_layerlog.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_layer_log_library(tmp_path):
    """A clean out-of-tree make of the library's own target: one translation unit, the shared export map, exactly the header's names as
    dynamic symbols, a gfx950 code object only and none of the packed fp32 forms test_build_cpu keeps out of the step's library."""
    build = str(tmp_path / "obj")
    so = os.path.join(build, "libmliis_layerlog.so")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, so], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "layerlog.o")) and "error" not in r.stderr.lower()
    assert "-fno-slp-vectorize" in r.stdout and "--version-script=exports.map" in r.stdout
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(LAYERLOG_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(LAYERLOG_OBJS\) \$\(LAYERLOG_TARGET\)", mk)


def test_layer_log_library_exports_its_header_and_answers_size_queries_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.LAYERLOG_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.LAYERLOG_SIGNATURES) == set(_dynamic_symbols(_lib.LAYERLOG_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.LAYERLOG_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES))
    assert _affected_packed_forms(_lib.LAYERLOG_LIB_PATH) == {}
    lib = _lib.layerlog_lib
    assert lib.load().mliis_layerlog_last_error() == b""
    assert lib.size("mliis_layerlog_record_words") == LL.RECORD_WORDS == 8 and LL.RECORD_DTYPE.itemsize == 32
    cq = lib.size("mliis_layerlog_chunk_quads")
    assert cq >= 64 and cq % 64 == 0
    one = lib.size("mliis_layerlog_workspace_bytes", 1)
    assert one >= 2 * 24 and one % 16 == 0 and lib.size("mliis_layerlog_workspace_bytes", 1012) == 1012 * one   # one partial per chunk
    assert lib.size("mliis_layerlog_workspace_bytes", 0) == 0 and lib.size("mliis_layerlog_workspace_bytes", -3) == 0
    # the entry point refuses what it can without touching a device: nothing is launched for a null pointer
    assert lib.load().mliis_layerlog_append(0, None, None, 8, None, 1, None, 1, None, 48, None, 1, None, 0, None) == -1
    assert lib.load().mliis_layerlog_last_error().startswith(b"layerlog_append:")


# ------------------------------------------------------------------------------------------------ the meta-learners, on a stub learner
H = 32
T_STUB = 5
STUB_NAMES = ["stub/t%d" % i for i in range(T_STUB)]


class LayerLoggedOracle(R.OracleLearner):
    """The CPU oracle with a step log and a per-tensor log: every inner_step writes a record and a row of T_STUB records into host rings
    exactly where the device would (slot = counter % capacity).  A row's x_l2 is 100 * step counter + tensor, so every row can be told
    apart; plant = (n-th load_task since construction, step of that task): that step's record and tensors 1 and 3 of its row are flagged
    non-finite -- the records only, the oracle's arithmetic stays finite."""

    def __init__(self, *a, step_log=64, plant=None, **kw):
        super().__init__(*a, **kw)
        self.step_log, self.layer_log, self.plant = int(step_log), True, plant
        self.layer_log_names = list(STUB_NAMES)
        self._ring = np.zeros((self.step_log, S.RECORD_WORDS), dtype=np.int32)
        self._layers = np.zeros((self.step_log, T_STUB, LL.RECORD_WORDS), dtype=np.int32)
        self._deltas = np.zeros((self.step_log, T_STUB), dtype=LL.RECORD_DTYPE)
        self._cursor = self._seen = self._loads = self._k = 0
        self._window = (0, 0)
        self.layer_reads = self.delta_reads = 0

    def load_task(self, images, labels):
        super().load_task(images, labels)
        self._loads += 1
        self._k = 0

    def inner_step(self, x, y=None, lr=None, **kw):
        loss = super().inner_step(x, y, lr=lr, **kw)
        bad = self.plant == (self._loads, self._k)
        slot = self._cursor % self.step_log
        self._ring.view(S.RECORD_DTYPE).reshape(self.step_log)[slot] = (loss, loss, 0.5, self.lr if lr is None else lr, 1.0, 0.5, 3 if bad else 0, 0)
        self._layers.view(LL.RECORD_DTYPE).reshape(self.step_log, T_STUB)[slot] = [
            (100.0 * self._cursor + t, 1.0 + (t * 7 + self._cursor) % 5, 2.0, 1.0, 2 if bad and t in (1, 3) else 0, 0,
             4 if bad and t in (1, 3) else LL.NONE, LL.NONE) for t in range(T_STUB)]
        self._cursor += 1
        self._k += 1
        return loss

    def read_step_log(self):
        out = S.decode(self._ring, self._cursor, self._seen)
        self._window = (self._seen, self._cursor)
        self._seen = self._cursor
        return out

    def read_layer_log(self, last_read=False):
        self.layer_reads += 1
        return LL.decode(self._layers, self._window[1], self._window[0]) if last_read else LL.decode(self._layers, self._cursor, self._seen)

    def layer_delta(self, a, b, row):
        d = (a - b).double()
        self._deltas[row] = [(float(d.norm()) + t, 0.0, float(b.double().norm()), 0.0, 0, 0, LL.NONE, LL.NONE) for t in range(T_STUB)]

    def read_layer_deltas(self, rows):
        self.delta_reads += 1
        return self._deltas[list(rows)].copy()


def _tasks(n, shots):
    return [metaseg.DeviceTask("t%d" % i, *[torch.tensor(a) for a in metaseg.synthetic_task(shots, H, seed=70 + i, block=4)]) for i in range(n)]


def _stub(**kw):
    return LayerLoggedOracle(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False, **kw)


STEP = dict(num_shots=4, inner_batch_size=2, inner_iters=2, replacement=False, meta_step_size=0.25, meta_batch_size=2)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


@pytest.mark.parametrize("fomaml", [False, True])
def test_meta_learner_reads_the_layer_rings_only_when_it_uses_them(fomaml):
    tasks = _tasks(3, 4)
    make = (lambda L, **kw: FOMLIS(L, train_shots=4, tail_shots=2, rng_mode="per_task", seed=2, **kw)) if fomaml else \
        (lambda L, **kw: Gecko(L, rng_mode="per_task", seed=2, **kw))
    plain = R.OracleLearner(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False)
    ref = _quiet(make, plain)
    L = _stub()
    theta0 = L.export_trainable().clone()
    meta = _quiet(make, L, step_log=True, layer_log=True, layer_log_interval=2)
    rows = []
    meta.inner_loop_layers_sink = rows.append
    for i in range(3):
        _quiet(ref.train_step, tasks, **STEP)
        _quiet(meta.train_step, tasks, **STEP)
        assert L.layer_reads == L.delta_reads == (1, 1, 2)[i]                 # iterations 0 and 2 read the rings, iteration 1 does not
    assert torch.equal(L.export_trainable(), plain.export_trainable())          # the update is the one without any log
    assert [r["meta_iter"] for r in rows] == [0, 2] and rows[1] is meta.inner_loop_layers_summary
    r0 = rows[0]
    # records 0..3 of iteration 0: task 0 took steps 0 and 1, task 1 steps 2 and 3
    assert r0["tasks"] == 2 and r0["grad_l2_first"] == [100.0 + t for t in range(T_STUB)] and r0["grad_l2_last"] == [200.0 + t for t in range(T_STUB)]
    assert r0["grad_absmax"] == [float(max(1.0 + (t * 7 + c) % 5 for c in range(4))) for t in range(T_STUB)]
    assert r0["first_nonfinite"] is None and all(len(r0[k]) == T_STUB for k in ("grad_to_weight_last", "delta_l2", "delta_rel"))
    # the delta is taken against the parameters the meta-iteration started from, with FOMAML too: tensor t's stub value is ||.|| + t
    assert r0["delta_l2"][3] - r0["delta_l2"][0] == pytest.approx(3.0) and r0["delta_l2"][0] > 0
    assert r0["delta_rel"][0] == pytest.approx(r0["delta_l2"][0] / float(theta0.double().norm()), rel=1e-6)
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        make(plain, step_log=True, layer_log=True)
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        make(_stub(), step_log=True, layer_log=True, layer_log_interval=0)


def test_a_non_finite_step_is_attributed_in_any_iteration_and_abort_carries_it():
    tasks = _tasks(3, 4)
    L = _stub(plant=(4, 1))                                                     # 4th load = iteration 1 (not a logging one), task 1, step 1
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=2, step_log=True, layer_log=True, layer_log_interval=100)
    rows = []
    meta.inner_loop_layers_sink = rows.append
    for _ in range(3):
        _quiet(meta.train_step, tasks, **STEP)
    assert [r["meta_iter"] for r in rows] == [0, 1] and L.layer_reads == 2
    assert rows[0]["first_nonfinite"] is None
    assert rows[1]["first_nonfinite"] == {"task": 1, "step": 1, "grad_nonfinite": (2, ["stub/t1", "stub/t3"]), "theta_nonfinite": (0, []),
                                          "largest_grads": rows[1]["first_nonfinite"]["largest_grads"]}
    amax = [1.0 + (t * 7 + 6) % 5 for t in range(T_STUB)]                        # the row of counter 6: task 1's step 0 of iteration 1
    order = sorted(range(T_STUB), key=lambda t: (-amax[t], t))[:3]
    assert rows[1]["first_nonfinite"]["largest_grads"] == [(STUB_NAMES[t], amax[t]) for t in order]
    # abort: the error names the tensors; a bad step 0 has no finite step before it
    L = _stub(plant=(1, 0))
    theta0 = L.export_trainable().clone()
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=2, on_divergence="abort", layer_log=True)
    with pytest.raises(S.DivergenceError, match="task 0 step 0") as ei, contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **STEP)
    e = ei.value
    assert e.grad_nonfinite == (2, ["stub/t1", "stub/t3"]) and e.theta_nonfinite == (0, []) and e.largest_grads is None
    assert "stub/t1, stub/t3" in str(e) and torch.equal(L.export_trainable(), theta0)
    # without the layer log the message is the one it always was
    L = _stub(plant=(1, 0))
    L.layer_log = False
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=2, on_divergence="abort")
    with pytest.raises(S.DivergenceError) as ei, contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **STEP)
    assert str(ei.value) == str(S.DivergenceError(0, 0, 0)) and ei.value.grad_nonfinite is None and L.layer_reads == 0


def test_small_rings_and_lanes_give_the_row_of_one_big_ring():
    tasks = _tasks(3, 4)
    step = dict(STEP, meta_batch_size=5)
    big = _stub()
    ref = _quiet(Gecko, big, rng_mode="per_task", seed=4, step_log=True, layer_log=True)
    _quiet(ref.train_step, tasks, **step)
    want = ref.inner_loop_layers_summary
    assert want["tasks"] == 5 and big.layer_reads == 1
    small = _stub(step_log=4)                                                   # two tasks of two steps fit, the third needs room
    meta = _quiet(Gecko, small, rng_mode="per_task", seed=4, step_log=True, layer_log=True)
    _quiet(meta.train_step, tasks, **step)
    assert small.layer_reads == 3 and meta.inner_loop_layers_summary == want
    # over lanes every learner's rows go to the tasks it ran: the per-task deltas are those of the task-by-task loop
    main, lanes = _stub(), [_stub(), _stub()]
    meta = _quiet(Gecko, main, rng_mode="per_task", seed=4, step_log=True, layer_log=True, lanes=lanes)
    _quiet(meta.train_step, tasks, **step)
    got = meta.inner_loop_layers_summary
    assert got["tasks"] == 5 and got["delta_l2"] == pytest.approx(want["delta_l2"], rel=1e-12) and got["delta_rel"] == pytest.approx(want["delta_rel"], rel=1e-12)


def test_train_gecko_writes_the_layer_file_beside_the_untouched_ones(tmp_path):
    tasks = _tasks(3, 4)
    kw = dict(num_shots=4, inner_batch_size=2, inner_iters=2, meta_batch_size=2, meta_iters=3, eval_interval=0, verbose=False, seed=2,
              meta_step_size=0.25, meta_step_size_final=0.25)
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "layers")
    for d, log in ((d0, dict(inner_loop_log=True)), (d1, dict(inner_loop_layer_log=True, inner_loop_layer_log_interval=2))):
        random.seed(11)              # (one rank: the tasks are drawn from the global generator, like the reference)
        np.random.seed(11)
        _quiet(train_gecko, _stub(), tasks, tasks, d, **log, **kw)
    assert sorted(os.listdir(os.path.join(d0, "train"))) == ["inner_loop.jsonl", "scalars.jsonl"]
    assert sorted(os.listdir(os.path.join(d1, "train"))) == ["inner_loop.jsonl", "inner_loop_layers.jsonl", "inner_loop_layers.names.json",
                                                             "scalars.jsonl"]
    for f in ("inner_loop.jsonl", "scalars.jsonl"):
        assert open(os.path.join(d0, "train", f)).read() == open(os.path.join(d1, "train", f)).read()
    rows = [json.loads(ln) for ln in open(os.path.join(d1, "train", "inner_loop_layers.jsonl"))]
    assert [r["meta_iter"] for r in rows] == [0, 2] and all(len(r["grad_l2_last"]) == T_STUB and r["tasks"] == 2 for r in rows)
    assert json.load(open(os.path.join(d1, "train", "inner_loop_layers.names.json"))) == STUB_NAMES
