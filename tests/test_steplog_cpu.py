"""The inner loop's step log, the host half: libmliis_steplog.so's build and exported ABI against include/mliis_steplog.h, the record decoder
and the per-meta-iteration summary (mliis_amd/steplog.py) on hand-made records, the divergence guard of Gecko / train_gecko on a stub
learner that wraps the CPU oracle and emits records (one of them planted non-finite), the guard's collective decision under gloo with two
ranks, and run_metasegnet.main with --inner-loop-log."""
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
from mliis_amd import metaseg
from mliis_amd import steplog as S
from mliis_amd.reptile import FOMLIS, Gecko
from mliis_amd.train import train_gecko
from oracle import efficientlab_ref as R
from test_build_cpu import _affected_packed_forms, _dynamic_symbols
from test_meta_cpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
H = 32
NAMES = {"mliis_steplog_last_error", "mliis_steplog_workspace_bytes", "mliis_steplog_record_words", "mliis_steplog_append"}


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_steplog.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_step_log_library(tmp_path):
    """A clean out-of-tree make of the library's own target: one translation unit, the shared export map, only mliis_* dynamic symbols, a
    gfx950 code object and none of the packed fp32 forms test_build_cpu keeps out of the step's library."""
    build = str(tmp_path / "obj")
    so = os.path.join(build, "libmliis_steplog.so")
    r = subprocess.run(["make", "-C", CSRC, "BUILD=" + build, so], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "steplog.o")) and "error" not in r.stderr.lower()
    assert "-fno-slp-vectorize" in r.stdout and "--version-script=exports.map" in r.stdout
    syms = _dynamic_symbols(so)
    assert syms and all(s.startswith("mliis_") for s in syms) and set(syms) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    # `all` builds it and `clean` removes it
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(STEPLOG_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(STEPLOG_OBJS\) \$\(STEPLOG_TARGET\)", mk)


def test_step_log_library_exports_its_header_and_answers_size_queries_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.STEPLOG_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    syms = set(_dynamic_symbols(_lib.STEPLOG_LIB_PATH))
    assert set(decls) == set(_lib.STEPLOG_SIGNATURES) == syms == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.STEPLOG_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES))
    assert _affected_packed_forms(_lib.STEPLOG_LIB_PATH) == {}
    assert _lib.steplog_lib.load().mliis_steplog_last_error() == b""
    assert _lib.steplog_lib.size("mliis_steplog_record_words") == S.RECORD_WORDS == 8 and S.RECORD_DTYPE.itemsize == 32
    ws = _lib.steplog_lib.size("mliis_steplog_workspace_bytes")
    assert ws >= 256 * 24 and ws % 16 == 0      # one partial (a double, a float, two counts) per workgroup of the fixed grid


# ------------------------------------------------------------------------------------------------ decoder and summary
def _ring_after(n_steps, capacity):
    """What the device leaves after n_steps appends into an empty ring: record k (loss = k) in slot k % capacity."""
    ring = np.zeros((capacity, 8), dtype=np.int32)
    rec = ring.view(S.RECORD_DTYPE).reshape(capacity)
    for k in range(n_steps):
        rec[k % capacity] = (float(k), 0.5 * k, 0.25, 1e-3, 2.0 * k, 3.0 * k, 0, 0)
    return ring


def test_decode_orders_across_the_wrap_and_counts_what_was_dropped():
    r, dropped = S.decode(_ring_after(3, 4), 3, 0)
    assert r.dtype == S.RECORD_DTYPE and list(r["loss"]) == [0.0, 1.0, 2.0] and dropped == 0 and list(r["grad_l2"]) == [0.0, 2.0, 4.0]
    r, dropped = S.decode(_ring_after(6, 4), 6, 3)           # slots 3, 0, 1: the read crosses the wrap
    assert list(r["loss"]) == [3.0, 4.0, 5.0] and dropped == 0
    r, dropped = S.decode(_ring_after(6, 4), 6, 0)           # six steps into four slots: the two oldest are gone
    assert list(r["loss"]) == [2.0, 3.0, 4.0, 5.0] and dropped == 2
    r, dropped = S.decode(_ring_after(6, 4), 6, 6)
    assert len(r) == 0 and dropped == 0
    r, dropped = S.decode(_ring_after(11, 3), 11, 1)         # a capacity that is no power of two
    assert list(r["loss"]) == [8.0, 9.0, 10.0] and dropped == 7
    # the device counter is 32 bits wide: the difference is taken modulo 2^32 (power-of-two ring: the slots continue across the wrap)
    ring = np.zeros((4, 8), dtype=np.int32)
    rec = ring.view(S.RECORD_DTYPE).reshape(4)
    for k, pos in enumerate(((1 << 32) - 2, (1 << 32) - 1, 0, 1)):
        rec[pos % 4]["loss"] = 10.0 + k
    r, dropped = S.decode(ring, 2, (1 << 32) - 2)
    assert list(r["loss"]) == [10.0, 11.0, 12.0, 13.0] and dropped == 0
    # int32 words as they come back from the device, counts above 2^31 included
    ring = np.zeros((1, 8), dtype=np.int32)
    ring[0, 6], ring[0, 7] = -1, 7
    r, _ = S.decode(ring, 1, 0)
    assert int(r["grad_nonfinite"][0]) == 0xFFFFFFFF and int(r["theta_nonfinite"][0]) == 7
    assert S.capacity_for(1) == 64 and S.capacity_for(64) == 64 and S.capacity_for(65) == 128 and S.capacity_for(200) == 256


def _records(rows):
    r = np.zeros(len(rows), dtype=S.RECORD_DTYPE)
    for k, row in enumerate(rows):
        r[k] = row
    return r


def test_attribution_by_issue_order_and_the_summary():
    recs = _records([(4.0, 4.0, 0.1, 1e-3, 8.0, 1.0, 0, 0), (3.0, 3.0, 0.2, 1e-3, 6.0, 2.0, 0, 0),
                     (2.0, 2.0, 0.3, 1e-3, 4.0, 9.0, 0, 0), (1.0, 1.0, 0.4, 2e-3, 2.0, 3.0, 0, 0)])
    one = S.split_tasks(recs, 1, 4)                              # T = 1: a task is one record
    assert [list(t["loss"]) for t in one] == [[4.0], [3.0], [2.0], [1.0]]
    four = S.split_tasks(recs, 4, 1)                             # T = 4: one task holds them all
    assert len(four) == 1 and list(four[0]["loss"]) == [4.0, 3.0, 2.0, 1.0]
    two = S.split_tasks(recs, 2, 2)
    assert [list(t["loss"]) for t in two] == [[4.0, 3.0], [2.0, 1.0]]
    for bad in (dict(steps_per_task=3, n_tasks=1), dict(steps_per_task=2, n_tasks=2, dropped=1), dict(steps_per_task=0, n_tasks=4)):
        with pytest.raises(ValueError):
            S.split_tasks(recs, **bad)
    # two tasks of two steps, handed over out of order (a lane finished the later task first)
    row = S.summarize([(3, two[1]), (1, two[0])], meta_iter=7)
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    assert row["meta_iter"] == 7 and row["tasks"] == 2 and row["steps"] == 4 and row["skipped"] is False
    assert row["loss_first"] == 3.0 and row["loss_last"] == 2.0                  # means of (4, 2) and of (3, 1)
    assert row["iou_first"] == (f32(0.1) + f32(0.3)) / 2 and row["iou_last"] == (f32(0.2) + f32(0.4)) / 2
    assert row["grad_l2_first"] == 6.0 and row["grad_l2_last"] == 4.0 and row["grad_absmax"] == 9.0
    assert row["lr"] == f32(2e-3)                                                # the last step of the last task
    assert row["nonfinite_steps"] == 0 and row["first_nonfinite"] is None
    assert all(v is None or isinstance(v, (int, float, bool, dict)) for v in row.values())
    json.dumps(row)
    # T = 1 and T = 4 summaries
    row1 = S.summarize(list(enumerate(one)))
    assert row1["tasks"] == 4 and row1["loss_first"] == row1["loss_last"] == 2.5
    row4 = S.summarize([(0, four[0])])
    assert row4["loss_first"] == 4.0 and row4["loss_last"] == 1.0 and row4["grad_absmax"] == 9.0


def test_the_first_non_finite_step_is_named_in_task_order():
    clean = (1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0)
    t0 = _records([clean, clean, clean])
    t1 = _records([clean, (1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 2), (float("nan"), 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0)])
    t2 = _records([(float("inf"), 1.0, 0.5, 1e-3, 1.0, 1.0, 0, 0), clean, (1.0, 1.0, 0.5, 1e-3, 1.0, 1.0, 5, 0)])
    assert list(S.nonfinite_steps(t1)) == [False, True, True] and list(S.nonfinite_steps(t2)) == [True, False, True]
    row = S.summarize([(2, t2), (0, t0), (1, t1)])
    assert row["nonfinite_steps"] == 4 and row["first_nonfinite"] == {"task": 1, "step": 1}
    assert np.isnan(row["loss_last"])                            # a NaN last loss stays visible in the mean ...
    line = json.dumps({k: S._json_number(v) for k, v in row.items()})
    assert "NaN" not in line and json.loads(line)["loss_last"] == "nan"   # ... and is written as strict JSON
    e = S.DivergenceError(12, 1, 1, rank=0)
    assert isinstance(e, RuntimeError) and (e.meta_iter, e.task, e.step) == (12, 1, 1) and "task 1 step 1" in str(e)
    assert "another rank" in str(S.DivergenceError(3, None, None, rank=1))


# ------------------------------------------------------------------------------------------------ the guard, on a stub learner
class LoggedOracle(R.OracleLearner):
    """The CPU oracle with a step log: every inner_step appends a record to a host ring exactly as the device does to its own (slot =
    counter % capacity).  plant = (n-th load_task since construction, step of that task): that one record gets a non-finite gradient
    count -- the record only, the oracle's arithmetic stays finite, so "off" can be compared with a run without any log."""

    def __init__(self, *a, step_log=64, plant=None, **kw):
        super().__init__(*a, **kw)
        self.step_log, self.plant = int(step_log), plant
        self._ring = np.zeros((self.step_log, S.RECORD_WORDS), dtype=np.int32)
        self._cursor = self._seen = self._loads = self._k = 0
        self.reads = 0

    def load_task(self, images, labels):
        super().load_task(images, labels)
        self._loads += 1
        self._k = 0

    def inner_step(self, x, y=None, lr=None, **kw):
        loss = super().inner_step(x, y, lr=lr, **kw)
        bad = self.plant == (self._loads, self._k)
        rec = self._ring.view(S.RECORD_DTYPE).reshape(self.step_log)
        rec[self._cursor % self.step_log] = (loss, loss, 0.5, self.lr if lr is None else lr, 1.0 + self._cursor, 0.5, 3 if bad else 0, 0)
        self._cursor += 1
        self._k += 1
        return loss

    def read_step_log(self):
        self.reads += 1
        out = S.decode(self._ring, self._cursor, self._seen)
        self._seen = self._cursor
        return out


def _tasks(n, shots):
    return [metaseg.DeviceTask("t%d" % i, *[torch.tensor(a) for a in metaseg.synthetic_task(shots, H, seed=70 + i, block=4)]) for i in range(n)]


def _stub(**kw):
    return LoggedOracle(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False, **kw)


STEP = dict(num_shots=4, inner_batch_size=2, inner_iters=2, replacement=False, meta_step_size=0.25, meta_batch_size=2)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = fn(*a, **kw)
    return out, buf.getvalue()


@pytest.mark.parametrize("fomaml", [False, True])
def test_guard_skip_abort_and_off_on_a_two_task_meta_batch(fomaml):
    tasks = _tasks(3, 4)
    make = (lambda L, **kw: FOMLIS(L, train_shots=4, tail_shots=2, rng_mode="per_task", seed=2, **kw)) if fomaml else \
        (lambda L, **kw: Gecko(L, rng_mode="per_task", seed=2, **kw))
    plain = R.OracleLearner(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False)
    ref, _ = _quiet(make, plain)
    _quiet(ref.train_step, tasks, **STEP)

    # off: the planted record is reported, the update is today's
    L = _stub(plant=(2, 1))
    theta0, bn0 = L.export_trainable().clone(), L.export_bn().clone()
    meta, _ = _quiet(make, L, step_log=True)
    assert meta.on_divergence == "off" and meta.step_log
    rows = []
    meta.inner_loop_sink = rows.append
    _quiet(meta.train_step, tasks, **STEP)
    assert torch.equal(L.export_trainable(), plain.export_trainable()) and torch.equal(L.export_bn(), plain.export_bn())
    assert not torch.equal(L.export_trainable(), theta0) and meta.meta_iter == 1
    row = meta.inner_loop_summary
    assert rows == [row] and row["tasks"] == 2 and row["steps"] == 4 and row["skipped"] is False and row["meta_iter"] == 0
    assert row["nonfinite_steps"] == 1 and row["first_nonfinite"] == {"task": 1, "step": 1}      # second load_task = task 1
    assert row["grad_l2_first"] == (1.0 + 3.0) / 2 and row["grad_l2_last"] == (2.0 + 4.0) / 2   # records attributed in issue order
    _quiet(meta.train_step, tasks, **STEP)                                                          # the next iteration is clean
    assert meta.inner_loop_summary["nonfinite_steps"] == 0 and meta.inner_loop_summary["meta_iter"] == 1 and len(rows) == 2

    # skip: parameters and BN tensors are bit-equal to before the iteration, the iteration still counts
    L = _stub(plant=(2, 1))
    meta, _ = _quiet(make, L, on_divergence="skip")
    assert meta.step_log                                                                            # implied
    _, out = _quiet(meta.train_step, tasks, **STEP)
    assert torch.equal(L.export_trainable(), theta0) and torch.equal(L.export_bn(), bn0)
    assert meta.meta_iter == 1 and meta.skipped_meta_iters == 1 and meta.inner_loop_summary["skipped"] is True
    assert out.count("skipped") == 1 and "task 1 step 1" in out
    _quiet(meta.train_step, tasks, **STEP)                                                          # and the run goes on
    assert meta.meta_iter == 2 and meta.skipped_meta_iters == 1 and not torch.equal(L.export_trainable(), theta0)

    # abort: DivergenceError names the task and the step; nothing was updated
    L = _stub(plant=(1, 0))
    meta, _ = _quiet(make, L, on_divergence="abort")
    with pytest.raises(S.DivergenceError, match="task 0 step 0") as ei, contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **STEP)
    assert (ei.value.meta_iter, ei.value.task, ei.value.step) == (0, 0, 0)
    assert torch.equal(L.export_trainable(), theta0) and torch.equal(L.export_bn(), bn0) and meta.meta_iter == 0


def test_a_ring_smaller_than_the_meta_batch_is_read_between_tasks_and_lanes_are_attributed():
    tasks = _tasks(3, 4)
    step = dict(STEP, meta_batch_size=5)
    big = _stub()
    ref, _ = _quiet(Gecko, big, rng_mode="per_task", seed=4, step_log=True)
    _quiet(ref.train_step, tasks, **step)
    assert big.reads == 2                                    # the discard at the head of the meta-batch, the read at its end
    small = _stub(step_log=4)                                # two tasks of two steps fit, the third needs room
    meta, _ = _quiet(Gecko, small, rng_mode="per_task", seed=4, step_log=True)
    _quiet(meta.train_step, tasks, **step)
    assert small.reads == 4 and meta.inner_loop_summary == ref.inner_loop_summary and ref.inner_loop_summary["steps"] == 10
    assert torch.equal(small.export_trainable(), big.export_trainable())
    # over lanes: every learner's records go to the tasks it ran, the losses are those of the task-by-task loop
    main, lanes = _stub(), [_stub(), _stub()]
    meta, _ = _quiet(Gecko, main, rng_mode="per_task", seed=4, step_log=True, lanes=lanes)
    _quiet(meta.train_step, tasks, **step)
    for k in ("tasks", "steps", "loss_first", "loss_last", "iou_first", "lr", "nonfinite_steps"):
        assert meta.inner_loop_summary[k] == ref.inner_loop_summary[k], k
    # a ring that cannot hold one task, a learner without a log, a mode nobody knows
    with pytest.raises(ValueError, match="holds 1 records"), contextlib.redirect_stdout(io.StringIO()):
        Gecko(_stub(step_log=1), rng_mode="per_task", step_log=True).train_step(tasks, **STEP)
    plain = R.OracleLearner(image_size=H, seed=3, dtype=torch.float64, lr=1e-2, drop_connect=False)
    for kw in (dict(step_log=True), dict(on_divergence="skip"), dict(on_divergence="panic")):
        with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
            Gecko(plain, **kw)
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        Gecko(_stub(), step_log=True, lanes=[plain])


def test_train_gecko_writes_the_log_and_abort_leaves_no_checkpoint(tmp_path):
    tasks = _tasks(3, 4)
    kw = dict(num_shots=4, inner_batch_size=2, inner_iters=2, meta_batch_size=2, meta_iters=3, eval_interval=0, verbose=False, seed=2,
              meta_step_size=0.25, meta_step_size_final=0.25)
    d = str(tmp_path / "skip")
    meta, out = _quiet(train_gecko, _stub(plant=(4, 0)), tasks, tasks, d, on_divergence="skip", **kw)     # 4th load = iteration 1, task 1
    rows = [json.loads(ln) for ln in open(os.path.join(d, "train", "inner_loop.jsonl"))]
    assert [r["meta_iter"] for r in rows] == [0, 1, 2] and [r["skipped"] for r in rows] == [False, True, False]
    assert rows[1]["first_nonfinite"] == {"task": 1, "step": 0} and meta.meta_iter == 3 and meta.skipped_meta_iters == 1
    assert open(os.path.join(d, "train", "scalars.jsonl")).read() == ""
    assert any(f.startswith("model.ckpt") for f in os.listdir(d))
    d = str(tmp_path / "abort")
    with pytest.raises(S.DivergenceError), contextlib.redirect_stdout(io.StringIO()):
        train_gecko(_stub(plant=(1, 1)), tasks, tasks, d, on_divergence="abort", **kw)
    assert sorted(os.listdir(d)) == ["test", "train"]                                               # no checkpoint, no state file
    rows = [json.loads(ln) for ln in open(os.path.join(d, "train", "inner_loop.jsonl"))]
    assert len(rows) == 1 and rows[0]["nonfinite_steps"] == 1 and rows[0]["skipped"] is False
    d = str(tmp_path / "plain")                                                                     # without the option: no such file
    _quiet(train_gecko, _stub(), tasks, tasks, d, **kw)
    assert not os.path.exists(os.path.join(d, "train", "inner_loop.jsonl"))


# ------------------------------------------------------------------------------------------------ gloo, world size 2
def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L = _stub(plant=(1, 1) if rank == 1 else None)         # only rank 1's task is flagged
        theta0, bn0 = L.export_trainable().clone(), L.export_bn().clone()
        with contextlib.redirect_stdout(io.StringIO()):
            meta = Gecko(L, seed=1, on_divergence="skip")
            meta.train_step(_tasks(3, 4), **STEP)
        first = bool(torch.equal(L.export_trainable(), theta0) and torch.equal(L.export_bn(), bn0))
        row1 = dict(meta.inner_loop_summary)
        with contextlib.redirect_stdout(io.StringIO()):
            meta.train_step(_tasks(3, 4), **STEP)                   # a clean iteration: the all-reduce still pairs up
        q.put((rank, first, row1, meta.meta_iter, meta.skipped_meta_iters, L.export_trainable().numpy()))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_both_ranks_skip_when_one_rank_saw_it():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, first, row, meta_iter, skipped, _ in res:
        assert first and row["skipped"] is True and meta_iter == 2 and skipped == 1, rank
        assert row["tasks"] == 1 and row["nonfinite_steps"] == (1 if rank == 1 else 0)             # each rank's row holds its own tasks
    assert res[1][2]["first_nonfinite"] == {"task": 1, "step": 1} and res[0][2]["first_nonfinite"] is None
    np.testing.assert_array_equal(res[0][5], res[1][5])                                             # and the ranks stay in step


# ------------------------------------------------------------------------------------------------ flags and the whole program
def test_flags_default_off_and_on_divergence_implies_the_log():
    p = A.argument_parser()
    off = p.parse_args([])
    assert off.inner_loop_log is False and off.on_divergence == "off" and not A.inner_loop_log(off)
    ref = A.argument_parser(extensions=False)
    for flag in (["--inner-loop-log"], ["--on-divergence", "skip"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            ref.parse_args(flag)
    assert "step_log" not in A.model_kwargs(off) and "inner_loop_log" not in A.train_kwargs(off) and "on_divergence" not in A.train_kwargs(off)
    assert not A.inner_loop_log(ref.parse_args([])) and "step_log" not in A.model_kwargs(ref.parse_args([]))
    on = p.parse_args(["--inner-loop-log", "--inner-iters", "20"])
    assert A.model_kwargs(on)["step_log"] == 64 and A.train_kwargs(on)["inner_loop_log"] is True and A.train_kwargs(on)["on_divergence"] == "off"
    assert A.model_kwargs(p.parse_args(["--inner-loop-log", "--inner-iters", "100"]))["step_log"] == 128
    for mode in ("skip", "abort"):
        a = p.parse_args(["--on-divergence", mode])
        assert A.inner_loop_log(a) and A.model_kwargs(a)["step_log"] >= 64 and A.train_kwargs(a)["on_divergence"] == mode
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        p.parse_args(["--on-divergence", "maybe"])
    assert "inner_loop_log" not in A.evaluate_kwargs(on)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--inner-loop-log" in readme and "--on-divergence" in readme


def _factory(device=None, feature_extractor_name="efficientnet-b0", image_size=H, rsd=(2, 4), learning_rate=1e-3, l2=False, dice=False,
             label_smoothing=0.0, seed=0, step_log=0, **_ignored):
    torch.set_num_threads(4)
    kw = dict(name=feature_extractor_name, image_size=image_size, rsd=tuple(rsd or ()), seed=seed, dtype=torch.float32, lr=learning_rate, l2=l2,
              dice=dice, label_smoothing=label_smoothing, drop_connect=False)
    return LoggedOracle(step_log=step_log, **kw) if step_log else R.OracleLearner(**kw)


def test_main_with_inner_loop_log_writes_one_line_per_meta_iteration(tmp_path):
    import run_metasegnet
    base = ["--image_size", str(H), "--rsd", "2", "4", "--sgd", "--shots", "2", "--inner-batch", "2", "--inner-iters", "2", "--meta-batch", "2",
            "--eval-samples", "2", "--eval-iters", "1", "--eval-batch", "2", "--synthetic-tasks", "6", "--meta-step", "0.5",
            "--learning-rate", "0.01", "--skip-train-task-eval", "--meta-iters", "3", "--eval-interval", "2"]
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "logged")
    _quiet(run_metasegnet.main, base + ["--checkpoint", d0], learner_factory=_factory, device="cpu")
    _quiet(run_metasegnet.main, base + ["--checkpoint", d1, "--inner-loop-log"], learner_factory=_factory, device="cpu")
    assert not os.path.exists(os.path.join(d0, "train", "inner_loop.jsonl"))
    rows = [json.loads(ln) for ln in open(os.path.join(d1, "train", "inner_loop.jsonl"))]
    assert [r["meta_iter"] for r in rows] == [0, 1, 2] and all(r["tasks"] == 2 and r["steps"] == 4 and not r["skipped"] for r in rows)
    assert all(r["nonfinite_steps"] == 0 and r["lr"] == float(np.float32(0.01)) and r["loss_first"] > 0 for r in rows)
    for split in ("train", "test"):
        a, b = (open(os.path.join(d, split, "scalars.jsonl")).read() for d in (d0, d1))
        assert a == b and len(a.splitlines()) == 2                                                  # i = 0 and i = 2
    assert sorted(f for f in os.listdir(os.path.join(d1, "train"))) == ["inner_loop.jsonl", "scalars.jsonl"]
