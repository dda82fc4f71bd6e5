"""The inner loop's step log, host side: the record layout of csrc/steplog.hip (include/mliis_steplog.h), the decoder of the device ring,
the per-meta-iteration summary and the divergence guard's exception.  numpy only -- nothing here needs a device.

A learner built with step_log=CAPACITY appends one record per inner step to a ring of CAPACITY records in device memory
(Learner.read_step_log copies ring and cursor back and calls decode()).  Gecko / FOMLIS(step_log=True) attribute a learner's records to
its tasks by issue order -- T records per task -- and summarize() condenses the tasks of one meta-iteration into one JSON-ready row.
"""
from __future__ import annotations

import json
import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

RECORD_WORDS = 8
RECORD_DTYPE = np.dtype([("loss", "<f4"), ("ce", "<f4"), ("iou", "<f4"), ("lr", "<f4"), ("grad_l2", "<f4"), ("grad_absmax", "<f4"),
                         ("grad_nonfinite", "<u4"), ("theta_nonfinite", "<u4")])
assert RECORD_DTYPE.itemsize == 4 * RECORD_WORDS

ON_DIVERGENCE = ("off", "skip", "abort")
MIN_CAPACITY = 64


class DivergenceError(RuntimeError):
    """An inner step of this meta-iteration produced a non-finite loss, gradient or parameter (on_divergence="abort").  Raised before the
    meta-update, so the parameters -- and every checkpoint written so far -- are those of the last good iteration.
    .meta_iter, .task, .step: where the first such step was seen on the rank that raised (task / step None: another rank saw it).
    With the per-tensor log (layerlog.attribute), keyword only and None without it: .grad_nonfinite / .theta_nonfinite = (number of
    tensors whose gradient / parameters were non-finite at that step, the first eight names), .largest_grads = the three [(name,
    grad_absmax)] largest of the task's last finite step (None when step 0 was the bad one)."""

    def __init__(self, meta_iter: int, task: Optional[int], step: Optional[int], rank: int = 0, *, grad_nonfinite=None,
                 theta_nonfinite=None, largest_grads=None):
        self.meta_iter, self.task, self.step, self.rank = meta_iter, task, step, rank
        self.grad_nonfinite, self.theta_nonfinite, self.largest_grads = grad_nonfinite, theta_nonfinite, largest_grads
        where = "task {} step {} of rank {}".format(task, step, rank) if task is not None else "a task of another rank"
        msg = "inner loop diverged in meta-iteration {}: non-finite loss, gradient or parameters at {}".format(meta_iter, where)
        for what, hit in (("gradient", grad_nonfinite), ("parameters", theta_nonfinite)):
            if hit is not None:
                msg += "; {} non-finite in {} tensors{}".format(what, hit[0], (": " + ", ".join(hit[1])) if hit[1] else "")
        if largest_grads is not None:
            msg += "; largest |grad| of the last finite step: " + ", ".join("{} {:.3g}".format(n, v) for n, v in largest_grads)
        super().__init__(msg)


def capacity_for(steps_per_task: int) -> int:
    """Ring capacity for tasks of `steps_per_task` inner steps: that many records rounded up to a power of two, at least MIN_CAPACITY."""
    n = max(int(steps_per_task), 1)
    return max(MIN_CAPACITY, 1 << (n - 1).bit_length())


def decode_ring(ring, cursor: int, last_cursor: int, dtype: np.dtype, row: Optional[str] = None) -> Tuple[np.ndarray, int]:
    """The decoder of every device ring (this log's, layerlog.decode, clip.decode): (records, dropped) -- what was written between the
    counter values last_cursor and cursor, oldest first, as a `dtype` array, and how many of those the ring no longer holds (more were
    written than its capacity: the oldest are the ones lost).  The counters are taken modulo 2^32 like the device's.  row None: a ring
    of [capacity, words] 32-bit words, records [kept]; row "T": one of [capacity, T, words] (the letter names the axis in the error),
    records [kept, T]."""
    words, n = np.ascontiguousarray(np.asarray(ring)).view(np.uint32), dtype.itemsize // 4
    if row is None:
        words = words.reshape(-1, n)
        if words.shape[0] < 1:
            raise ValueError("empty ring")
    elif words.ndim != 3 or words.shape[2] != n or words.shape[0] < 1 or words.shape[1] < 1:
        raise ValueError("expected a [capacity, {}, {}] ring, got {}".format(row, n, words.shape))
    capacity = words.shape[0]
    new = (int(cursor) - int(last_cursor)) & 0xFFFFFFFF
    kept = min(new, capacity)
    pos = (int(cursor) - kept + np.arange(kept, dtype=np.int64)) & 0xFFFFFFFF
    return words[pos % capacity].copy().view(dtype).reshape((kept,) + words.shape[1:-1]), new - kept


def decode(ring, cursor: int, last_cursor: int = 0) -> Tuple[np.ndarray, int]:
    """(records, dropped): the records appended between the counter values last_cursor and cursor, oldest first, as a RECORD_DTYPE array,
    and how many of them the ring no longer holds (more were appended than its capacity: the oldest are the ones lost).  ring: the
    [capacity, 8] 32-bit words read back from the device; the counters are taken modulo 2^32 like the device's."""
    return decode_ring(ring, cursor, last_cursor, RECORD_DTYPE)


def nonfinite_steps(records: np.ndarray) -> np.ndarray:
    """bool per record: a non-finite loss, or non-finite elements in the gradient or in the parameters."""
    return ~np.isfinite(records["loss"]) | (records["grad_nonfinite"] > 0) | (records["theta_nonfinite"] > 0)


def split_tasks(records: np.ndarray, steps_per_task: int, n_tasks: int, dropped: int = 0) -> List[np.ndarray]:
    """A learner's records cut into its tasks by issue order: n_tasks runs of steps_per_task records.  A log that does not hold exactly
    those (records dropped by a ring that was too small, steps nobody accounted for) cannot be attributed and is an error."""
    T = int(steps_per_task)
    if T < 1 or dropped or len(records) != n_tasks * T:
        raise ValueError("step log holds {} records ({} dropped); {} tasks of {} steps were issued".format(len(records), dropped, n_tasks, T))
    return [records[k * T:(k + 1) * T] for k in range(n_tasks)]


def _mean(values) -> float:
    return float(np.mean(np.asarray(values, dtype=np.float64)))


def summarize(task_records: Sequence[Tuple[int, np.ndarray]], meta_iter: int = 0) -> dict:
    """One meta-iteration's row from [(task index, that task's records in step order)], the tasks of ONE rank: the mean over the tasks of
    the first and of the last step's loss / iou / grad_l2, the largest grad_absmax, the lr of the last step issued, the number of
    non-finite steps (nonfinite_steps) and the task and step of the first one in task order.  Plain Python numbers throughout."""
    tasks = sorted(task_records, key=lambda tr: tr[0])
    row = {"meta_iter": int(meta_iter), "tasks": len(tasks), "steps": int(sum(len(r) for _, r in tasks))}
    filled = [r for _, r in tasks if len(r)]
    for name in ("loss", "iou", "grad_l2"):
        row[name + "_first"] = _mean([r[name][0] for r in filled]) if filled else None
        row[name + "_last"] = _mean([r[name][-1] for r in filled]) if filled else None
    row["grad_absmax"] = float(max(float(r["grad_absmax"].max()) for r in filled)) if filled else None
    row["lr"] = float(filled[-1]["lr"][-1]) if filled else None
    row["nonfinite_steps"] = 0
    row["first_nonfinite"] = None
    for t, r in tasks:
        bad = np.flatnonzero(nonfinite_steps(r))
        row["nonfinite_steps"] += int(bad.size)
        if bad.size and row["first_nonfinite"] is None:
            row["first_nonfinite"] = {"task": int(t), "step": int(bad[0])}
    row["skipped"] = False
    return row


def _json_number(v):
    """JSON has no NaN / Infinity: a non-finite float is written as its name in a string."""
    if isinstance(v, float) and not math.isfinite(v):
        return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf")
    return v


class InnerLoopWriter:
    """<directory>/inner_loop.jsonl: one summarize() row per line, appended and flushed as it comes."""

    def __init__(self, directory: str):
        os.makedirs(directory, exist_ok=True)
        self.path = os.path.join(directory, "inner_loop.jsonl")
        self.f = open(self.path, "a")

    def add(self, row: dict):
        self.f.write(json.dumps({k: _json_number(v) for k, v in row.items()}) + "\n")
        self.f.flush()
