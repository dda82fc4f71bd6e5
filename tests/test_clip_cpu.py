"""The inner loop's gradient clipping, the host half: libmliis_clip.so's build and exported ABI against include/mliis_clip.h, the chunk
tables it shares with the per-tensor log at its own chunk size, the flags, the record decoder and the summary (mliis_amd/clip.py) on
hand-made records, and the meta-learners' use of the clip's ring on a stub learner that wraps the CPU oracle."""
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from mliis_amd import args as A
from mliis_amd import clip as CL
from mliis_amd import layerlog as LL
from mliis_amd import spec
from mliis_amd import steplog as S
from mliis_amd.reptile import FOMLIS, Gecko
from mliis_amd.train import train_gecko
from test_build_cpu import _affected_packed_forms, _dynamic_symbols
from test_steplog_cpu import STEP, LoggedOracle, _quiet, _tasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_clip_last_error", "mliis_clip_chunk_quads", "mliis_clip_workspace_bytes", "mliis_clip_record_words", "mliis_clip_apply"}
H = 32


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_clip.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_clip_library(tmp_path):
    """A clean out-of-tree `make BUILD=... all` links the library: one translation unit, the shared export map, exactly the header's names
    as dynamic symbols, a gfx950 code object only and none of the packed fp32 forms test_build_cpu keeps out of the step's library."""
    build = str(tmp_path / "obj")
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    r = subprocess.run(["make", "-C", CSRC, "-j" + jobs, "BUILD=" + build, "all"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    so = os.path.join(build, "libmliis_clip.so")
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "clip.o"))
    line = next(ln for ln in r.stdout.splitlines() if " clip.hip " in ln + " ")
    assert "-fno-slp-vectorize" in line and "--offload-arch=gfx950" in line
    assert any("--version-script=exports.map" in ln and "libmliis_clip.so" in ln for ln in r.stdout.splitlines())
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(CLIP_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(CLIP_OBJS\) \$\(CLIP_TARGET\)", mk)


def test_clip_library_exports_its_header_and_answers_size_queries_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.CLIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.CLIP_SIGNATURES) == set(_dynamic_symbols(_lib.CLIP_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.CLIP_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES) |
                             set(_lib.LAYERLOG_SIGNATURES))
    assert _affected_packed_forms(_lib.CLIP_LIB_PATH) == {}
    lib = _lib.clip_lib
    assert lib.load().mliis_clip_last_error() == b""
    assert lib.size("mliis_clip_record_words") == CL.RECORD_WORDS == 8 and CL.RECORD_DTYPE.itemsize == 32
    cq = lib.size("mliis_clip_chunk_quads")
    assert cq >= 64 and cq % 64 == 0
    one, many = lib.size("mliis_clip_workspace_bytes", 1, 1), lib.size("mliis_clip_workspace_bytes", 1012, 169)
    assert one % 16 == 0 and many % 16 == 0 and (many - one) % 1011 == 0 and (many - one) // 1011 >= 24        # one partial per chunk
    for nchunks, T in ((0, 1), (-3, 1), (4, 0), (4, -1)):
        assert lib.size("mliis_clip_workspace_bytes", nchunks, T) == 0
    # the entry point refuses what it can without touching a device: nothing is launched for a null pointer or a bad value
    raw = lib.load().mliis_clip_apply
    assert raw(0, None, None, 8, None, 1, None, 1, 1.0, 1e-3, None, one, None, 1, None, None) == -1
    assert lib.load().mliis_clip_last_error().startswith(b"clip_apply:")
    assert raw(2, None, None, 8, None, 1, None, 1, 1.0, 1e-3, None, one, None, 1, None, None) == -1
    assert b"mode" in lib.load().mliis_clip_last_error()


# ------------------------------------------------------------------------------------------------ the tables, at this library's chunk size
def _check_table(sizes, cq):
    """chunks tile every tensor's quads exactly once and in order, none crosses a tensor or exceeds the chunk size, valid elements sum to
    the sizes, tensors sit at the arena's padded offsets -- and the validator accepts the table."""
    t = LL.chunk_table(sizes, cq)
    assert t.n == sum((s + 3) // 4 * 4 for s in sizes) and t.segs.shape == (len(sizes), 4)
    off, next_chunk = 0, 0
    for k, size in enumerate(sizes):
        q0, count, c0, c1 = t.segs[k].tolist()
        quads = (size + 3) // 4
        assert q0 * 4 == off and count == size and c0 == next_chunk and c1 - c0 == (quads + cq - 1) // cq
        at, valid = q0, 0
        for c in range(c0, c1):
            ct, cq0, cquads, cvalid = t.chunks[c].tolist()
            assert ct == k and cq0 == at and 1 <= cquads <= cq and (cquads == cq or c == c1 - 1)
            assert 4 * cquads - 3 <= cvalid <= 4 * cquads
            at += cquads
            valid += cvalid
        assert at == q0 + quads and valid == size
        off += quads * 4
        next_chunk = c1
    assert next_chunk == len(t.chunks)
    LL.validate_table(t.chunks, t.segs, t.n, cq)
    return t


def test_tables_cross_every_edge_at_the_clip_chunk_size():
    from mliis_amd._lib import clip_lib
    cq = clip_lib.size("mliis_clip_chunk_quads")
    CH = 4 * cq
    t = _check_table([1, 3, 4, 5], cq)
    assert t.chunks.tolist() == [[0, 0, 1, 1], [1, 1, 1, 3], [2, 2, 1, 4], [3, 3, 2, 5]] and t.n == 20
    t = _check_table([CH], cq)                               # exactly one chunk
    assert t.chunks.tolist() == [[0, 0, cq, CH]]
    t = _check_table([CH + 1], cq)                           # one chunk + 1 quad, of which one element counts
    assert t.chunks.tolist() == [[0, 0, cq, CH], [0, cq, 1, 1]]
    t = _check_table([CH + 4, 1, CH - 1], cq)
    assert t.chunks.tolist() == [[0, 0, cq, CH], [0, cq, 1, 4], [1, cq + 1, 1, 1], [2, cq + 2, cq, CH - 1]]
    bad = t.chunks.copy()
    bad[1, 2] = 2                                            # a chunk that runs into the next tensor
    with pytest.raises(ValueError):
        LL.validate_table(bad, t.segs, t.n, cq)


@pytest.mark.parametrize("name,size,T", [("efficientnet-b0", 224, 169), ("efficientnet-b3", 384, 361)])
def test_tables_of_the_real_arenas(name, size, T):
    from mliis_amd._lib import clip_lib
    arch = spec.derive(name, size, [2, 4], 0.0, False, skip_decoding=False)
    sizes = [p.size for p in spec.param_table(arch) if p.trainable]
    assert len(sizes) == T
    t = _check_table(sizes, clip_lib.size("mliis_clip_chunk_quads"))
    assert clip_lib.size("mliis_clip_workspace_bytes", len(t.chunks), T) >= 32 * len(t.chunks)


# ------------------------------------------------------------------------------------------------ flags
def test_flags_become_learner_arguments_and_are_absent_by_default():
    p, ref = A.argument_parser(), A.argument_parser(extensions=False)
    off = p.parse_args([])
    assert off.inner_clip_norm is None and off.inner_clip_ratio is None and off.inner_clip_ratio_eps == 1e-3 and A.grad_clip(off) is None
    assert not any("clip" in k for k in A.model_kwargs(off)) and not any("clip" in k for k in A.train_kwargs(off))
    assert not any("clip" in k for k in A.model_kwargs(ref.parse_args([])))
    on = A.model_kwargs(p.parse_args(["--inner-clip-norm", "2.5", "--inner-iters", "100"]))
    assert on["grad_clip"] == ("norm", 2.5) and on["clip_log"] == S.capacity_for(100) == 128 and "step_log" not in on
    on = A.model_kwargs(p.parse_args(["--inner-clip-ratio", "0.05"]))
    assert on["grad_clip"] == ("ratio", 0.05, 1e-3) and on["clip_log"] == 64
    on = A.model_kwargs(p.parse_args(["--inner-clip-ratio", "0.05", "--inner-clip-ratio-eps", "1e-2", "--inner-loop-log"]))
    assert on["grad_clip"] == ("ratio", 0.05, 1e-2) and on["clip_log"] == on["step_log"] == 64
    assert not any("clip" in k for k in A.train_kwargs(p.parse_args(["--inner-clip-norm", "1"])))      # the learner carries it, lanes too
    with pytest.raises(ValueError, match="exclude"):
        A.model_kwargs(p.parse_args(["--inner-clip-norm", "1", "--inner-clip-ratio", "0.1"]))
    for flag in ("--inner-clip-norm", "--inner-clip-ratio", "--inner-clip-ratio-eps"):
        for bad in ("0", "-1", "nan", "inf", "x"):
            with pytest.raises(SystemExit), _quiet_stderr():
                p.parse_args([flag, bad])
        with pytest.raises(SystemExit), _quiet_stderr():                                                 # the reference's parser has none
            ref.parse_args([flag, "1"])
    for text in (open(os.path.join(ROOT, "README.md")).read(), p.format_help()):
        assert "--inner-clip-norm" in text and "--inner-clip-ratio" in text and "--inner-clip-ratio-eps" in text
    assert "outside the clip" in re.sub(r"\s+", " ", p.format_help())
    # Learner's own parser of the argument
    assert CL.parse(None) is None and CL.parse(("norm", 2)) == ("norm", 2.0, CL.DEFAULT_RATIO_EPS) and CL.parse(["ratio", 0.1]) == ("ratio", 0.1, 1e-3)
    for bad in (("norm",), ("norm", 1, 2), ("ratio", 0.1, 1e-3, 4), ("both", 1), ("norm", 0), ("norm", float("nan")), ("ratio", 0.1, -1), "norm", 3):
        with pytest.raises(ValueError):
            CL.parse(bad)


def _quiet_stderr():
    import contextlib
    import io
    return contextlib.redirect_stderr(io.StringIO())


# ------------------------------------------------------------------------------------------------ decode and summarize
def _rows(values):
    """[steps, R] records from (g_l2, ref, scale, nonfinite, flags) tuples."""
    a = np.zeros((len(values), len(values[0])), dtype=CL.RECORD_DTYPE)
    for k, row in enumerate(values):
        for r, (g, ref, s, nf, fl) in enumerate(row):
            a[k, r] = (g, ref, s, nf, fl, (0, 0, 0))
    return a


def test_decode_across_the_wrap_of_ring_and_counter():
    R = 2
    ring = np.zeros((4, R, 8), dtype=np.int32)
    rec = ring.view(CL.RECORD_DTYPE).reshape(4, R)
    for c in range(6):                                       # rows 0..5 written into a ring of 4: 4 and 5 overwrote 0 and 1
        rec[c % 4] = [(10.0 * c + r, 1.0, 0.5, 0, 1, (0, 0, 0)) for r in range(R)]
    got, dropped = CL.decode(ring, 6, 0)
    assert dropped == 2 and got.shape == (4, R) and got["g_l2"][:, 0].tolist() == [20.0, 30.0, 40.0, 50.0] and got["g_l2"][0, 1] == 21.0
    got, dropped = CL.decode(ring, 6, 3)
    assert dropped == 0 and got["g_l2"][:, 0].tolist() == [30.0, 40.0, 50.0]
    assert CL.decode(ring, 6, 6)[0].shape == (0, R)
    assert CL.decode(ring.view(np.float32), 6, 3)[0]["g_l2"][:, 0].tolist() == [30.0, 40.0, 50.0]     # any 32-bit view of the words
    # the counter wraps modulo 2^32: rows written at 2^32 - 2, 2^32 - 1, 0
    rec[(2 ** 32 - 2) % 4], rec[(2 ** 32 - 1) % 4], rec[0] = [(1.0, 1, 1, 0, 0, (0, 0, 0))] * R, [(2.0, 1, 1, 0, 0, (0, 0, 0))] * R, [(3.0, 1, 1, 0, 0, (0, 0, 0))] * R
    got, dropped = CL.decode(ring, 1, 2 ** 32 - 2)
    assert dropped == 0 and got["g_l2"][:, 0].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        CL.decode(np.zeros((4, 8), dtype=np.int32), 1, 0)


def test_summarize_on_hand_made_records_with_a_bypassed_step():
    C, B = CL.CLIPPED, CL.BYPASSED
    t0 = _rows([[(4.0, 2.0, 0.5, 0, C)], [(1.0, 2.0, 1.0, 0, 0)], [(8.0, 2.0, 0.25, 0, C)]])
    t1 = _rows([[(2.0, 2.0, 1.0, 0, 0)], [(3.0, 2.0, 1.0, 7, B)], [(16.0, 2.0, 0.125, 0, C)]])
    row = CL.summarize([(1, t1), (0, t0)])
    assert row == dict(clip_frac=0.5, clip_scale_min=0.125, grad_l2_preclip_first=3.0, grad_l2_preclip_last=12.0, clip_bypassed=1)
    json.dumps(row)
    assert CL.clipped_steps(t1).tolist() == [False, False, True] and CL.bypassed_steps(t1).tolist() == [False, True, False]
    # per tensor: a step counts once however many tensors clipped; the whole gradient's norm is sqrt(sum of squares)
    r = _rows([[(3.0, 1.0, 1 / 3, 0, C), (4.0, 9.0, 1.0, 0, 0)], [(0.3, 1.0, 1.0, 0, 0), (0.4, 9.0, 1.0, 0, 0)]])
    row = CL.summarize([(0, r)])
    assert row["clip_frac"] == 0.5 and row["clip_scale_min"] == pytest.approx(1 / 3) and row["grad_l2_preclip_first"] == pytest.approx(5.0)
    assert row["grad_l2_preclip_last"] == pytest.approx(0.5) and row["clip_bypassed"] == 0
    empty = CL.summarize([])
    assert empty == dict(clip_frac=None, clip_scale_min=None, grad_l2_preclip_first=None, grad_l2_preclip_last=None, clip_bypassed=0)
    assert set(empty) == set(row)


# ------------------------------------------------------------------------------------------------ the meta-learners, on a stub learner
CLIP_KEYS = {"clip_frac", "clip_scale_min", "grad_l2_preclip_first", "grad_l2_preclip_last", "clip_bypassed"}


class ClippedOracle(LoggedOracle):
    """The CPU oracle with a step log and a clip ring (one record per step, as by global norm): every inner_step writes a row exactly where
    the device would.  Step counter c: g_l2 = 4 + c against ref 6, so steps 3, 4, ... are flagged clipped; `events` lists every ring read."""

    def __init__(self, *a, clip=True, **kw):
        super().__init__(*a, **kw)
        self.grad_clip = ("norm", 6.0, 1e-3) if clip else None
        self.clip_log = self.step_log if clip else 0
        self._clip_ring = np.zeros((self.step_log, 1, CL.RECORD_WORDS), dtype=np.int32)
        self._window = (0, 0)
        self.events = []

    def inner_step(self, x, y=None, lr=None, **kw):
        c = self._cursor
        g = 4.0 + c
        self._clip_ring.view(CL.RECORD_DTYPE).reshape(self.step_log, 1)[c % self.step_log, 0] = (
            g, 6.0, min(1.0, 6.0 / g), 0, CL.CLIPPED if g > 6.0 else 0, (0, 0, 0))
        return super().inner_step(x, y, lr=lr, **kw)

    def skip_step_log(self):
        self._seen = self._cursor

    def read_step_log(self):
        self.events.append("step")
        self._window = (self._seen, self._cursor)
        return super().read_step_log()

    def read_clip_log(self, last_read=False):
        assert last_read, "the meta-learner reads the clip's ring from the copy the step log's read fetched"
        self.events.append("clip")
        return CL.decode(self._clip_ring, self._window[1], self._window[0])


def _stub(**kw):
    return ClippedOracle(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False, **kw)


@pytest.mark.parametrize("fomaml", [False, True])
def test_meta_learner_reads_the_clip_ring_only_where_it_reads_the_step_ring(fomaml):
    tasks = _tasks(3, 4)
    make = (lambda L, **kw: FOMLIS(L, train_shots=4, tail_shots=2, rng_mode="per_task", seed=2, **kw)) if fomaml else \
        (lambda L, **kw: Gecko(L, rng_mode="per_task", seed=2, **kw))
    L, plain = _stub(), _stub(clip=False)
    meta, ref = _quiet(make, L, step_log=True)[0], _quiet(make, plain, step_log=True)[0]
    assert meta.clip_log and not ref.clip_log
    for _ in range(2):
        _quiet(meta.train_step, tasks, **STEP)
        _quiet(ref.train_step, tasks, **STEP)
    assert L.events == ["step", "clip"] * 2 and plain.events == ["step"] * 2
    row, base = meta.inner_loop_summary, ref.inner_loop_summary
    assert set(row) == set(base) | CLIP_KEYS and not CLIP_KEYS & set(base) and {k: row[k] for k in base} == base
    # iteration 1: counters 4..7, g_l2 8..11, all clipped; task 0 took 4 and 5, task 1 took 6 and 7
    assert row["clip_frac"] == 1.0 and row["clip_scale_min"] == pytest.approx(6.0 / 11.0) and row["clip_bypassed"] == 0
    assert row["grad_l2_preclip_first"] == 9.0 and row["grad_l2_preclip_last"] == 10.0
    assert torch.equal(L.export_trainable(), plain.export_trainable())
    # a small ring is read -- step ring first, clip ring right behind it -- before the steps that would overwrite it
    small = _stub(step_log=4)
    meta4 = _quiet(make, small, step_log=True)[0]
    _quiet(meta4.train_step, tasks, **dict(STEP, meta_batch_size=5))
    assert small.events == ["step", "clip"] * 3
    big = _stub()
    meta_big = _quiet(make, big, step_log=True)[0]
    _quiet(meta_big.train_step, tasks, **dict(STEP, meta_batch_size=5))
    assert big.events == ["step", "clip"] and meta4.inner_loop_summary == meta_big.inner_loop_summary
    assert meta_big.inner_loop_summary["clip_frac"] == 0.7          # counters 0..9: g_l2 4..13, seven of them above 6
    # without the step log the clip's ring is never read
    quiet = _stub()
    m = _quiet(make, quiet)[0]
    _quiet(m.train_step, tasks, **STEP)
    assert quiet.events == [] and not m.clip_log
    # a lane without clipping beside a learner with it is refused; so is a clip ring smaller than the step ring
    with pytest.raises(ValueError, match="grad_clip"):
        _quiet(make, _stub(), step_log=True, lanes=[_stub(clip=False)])
    short = _stub()
    short.clip_log = 8
    with pytest.raises(ValueError, match="clip ring"):
        _quiet(make, short, step_log=True)


def test_train_gecko_adds_the_clip_keys_to_inner_loop_jsonl_only_with_clipping(tmp_path):
    tasks = _tasks(3, 4)
    kw = dict(num_shots=4, inner_batch_size=2, inner_iters=2, meta_batch_size=2, meta_iters=2, eval_interval=0, verbose=False, seed=2,
              meta_step_size=0.25, meta_step_size_final=0.25, inner_loop_log=True)
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "clip")
    for d, clip in ((d0, False), (d1, True)):
        random.seed(11)
        np.random.seed(11)
        _quiet(train_gecko, _stub(clip=clip), tasks, tasks, d, **kw)
    assert sorted(os.listdir(os.path.join(d0, "train"))) == sorted(os.listdir(os.path.join(d1, "train"))) == ["inner_loop.jsonl", "scalars.jsonl"]
    assert open(os.path.join(d0, "train", "scalars.jsonl")).read() == open(os.path.join(d1, "train", "scalars.jsonl")).read()
    plain = [json.loads(ln) for ln in open(os.path.join(d0, "train", "inner_loop.jsonl"))]
    clip = [json.loads(ln) for ln in open(os.path.join(d1, "train", "inner_loop.jsonl"))]
    assert len(plain) == len(clip) == 2
    for a, b in zip(plain, clip):
        assert not CLIP_KEYS & set(a) and set(b) == set(a) | CLIP_KEYS and {k: b[k] for k in a} == a
    assert clip[0]["clip_frac"] == 0.25 and clip[1]["clip_frac"] == 1.0 and clip[0]["clip_scale_min"] == pytest.approx(6.0 / 7.0)
