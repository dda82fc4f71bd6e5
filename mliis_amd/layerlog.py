"""The inner loop's per-tensor log, host side: the chunk table of csrc/layerlog.hip (include/mliis_layerlog.h) as a pure function of the
tensor sizes, its validator, the record layout, the decoder of the device ring, the attribution of a non-finite step to tensors and the
per-meta-iteration summary.  numpy only -- nothing here needs a device.

A learner built with step_log=CAPACITY, layer_log=True writes one row of T records (T trainable tensors, arena order) per inner step into
a ring of CAPACITY rows; row k belongs to the same step as record k of the step log (steplog.py), so the two are decoded with the same
cursors and cut into tasks the same way.
"""
from __future__ import annotations

import json
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .steplog import _json_number, decode_ring, nonfinite_steps

RECORD_WORDS = 8
# step mode: x = the gradient, y = the parameters; delta mode: x = a - b, y = b
RECORD_DTYPE = np.dtype([("x_l2", "<f4"), ("x_absmax", "<f4"), ("y_l2", "<f4"), ("y_absmax", "<f4"), ("x_nonfinite", "<u4"),
                         ("y_nonfinite", "<u4"), ("x_first", "<u4"), ("y_first", "<u4")])
assert RECORD_DTYPE.itemsize == 4 * RECORD_WORDS
NONE = 0xFFFFFFFF          # x_first / y_first of a tensor without a non-finite element
MODES = {"step": 0, "delta": 1}
NAMES_SHOWN = 8            # tensor names a divergence report lists
LARGEST_SHOWN = 3


class ChunkTable(NamedTuple):
    chunks: np.ndarray     # int32 [nchunks, 4]: tensor, first quad of the arena, quads, valid elements
    segs: np.ndarray       # int32 [T, 4]: first quad, element count, first chunk, one past the last chunk
    n: int                 # floats of the arena the table covers (every tensor padded to a multiple of 4)


def chunk_table(sizes: Sequence[int], chunk_quads: int) -> ChunkTable:
    """The work of the first launch for an arena that packs tensors of `sizes` elements in order, each padded to a multiple of 4 floats
    (arena.Arena's layout): every tensor cut into chunks of at most chunk_quads 16-byte quads, consecutive and ascending; a chunk's valid
    elements are 4 * quads but for the tensor's last chunk, which stops at the tensor's count (its padding is read into nothing)."""
    cq = int(chunk_quads)
    if cq < 1:
        raise ValueError("chunk_quads = {}".format(chunk_quads))
    if len(sizes) < 1:
        raise ValueError("no tensor")
    chunks, segs, quad = [], [], 0
    for t, size in enumerate(sizes):
        size = int(size)
        if size < 1:
            raise ValueError("tensor {} has {} elements".format(t, size))
        quads, first = (size + 3) // 4, len(chunks)
        for q0 in range(0, quads, cq):
            q = min(cq, quads - q0)
            chunks.append((t, quad + q0, q, min(4 * q, size - 4 * q0)))
        segs.append((quad, size, first, len(chunks)))
        quad += quads
    if quad > 0x7FFFFFFF:
        raise ValueError("arena of {} quads: the tables address quads with 32 bits".format(quad))
    return ChunkTable(np.asarray(chunks, dtype=np.int32).reshape(-1, 4), np.asarray(segs, dtype=np.int32).reshape(-1, 4), 4 * quad)


def validate_table(chunks, segs, n: int, chunk_quads: int) -> None:
    """ValueError unless the tables are ones the kernels may follow inside arenas of n floats: int32 [.., 4] arrays, tensors ascending and
    non-overlapping inside n, counts >= 1, chunk ranges contiguous from 0 to nchunks, and each tensor's chunks tiling its quads exactly,
    in order, none longer than chunk_quads, with valid elements that sum to the tensor's count."""
    chunks, segs = np.asarray(chunks), np.asarray(segs)
    for name, a in (("chunks", chunks), ("segs", segs)):
        if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1:
            raise ValueError("{}: expected a non-empty int32 [.., 4] array, got {} {}".format(name, a.dtype, a.shape))
    n, cq = int(n), int(chunk_quads)
    if n < 4 or n % 4 or cq < 1:
        raise ValueError("n = {} (a positive multiple of 4), chunk_quads = {}".format(n, cq))
    end_quad, next_chunk = 0, 0
    for t, (q0, count, c0, c1) in enumerate(segs.tolist()):
        if count < 1:
            raise ValueError("tensor {}: {} elements".format(t, count))
        quads = (count + 3) // 4
        if q0 < end_quad:
            raise ValueError("tensor {}: first quad {} is below the end of the tensor before it ({}): not ascending / overlapping".format(t, q0, end_quad))
        if (q0 + quads) * 4 > n:
            raise ValueError("tensor {}: quads [{}, {}) leave the arena of {} floats".format(t, q0, q0 + quads, n))
        end_quad = q0 + quads
        if c0 != next_chunk or c1 <= c0 or c1 > chunks.shape[0]:
            raise ValueError("tensor {}: chunk range [{}, {}) does not continue at {} inside {} chunks".format(t, c0, c1, next_chunk, chunks.shape[0]))
        next_chunk = c1
        at, left = q0, count
        for c in range(c0, c1):
            ct, cq0, cquads, valid = chunks[c].tolist()
            if ct != t or cq0 != at or not 1 <= cquads <= cq or at + cquads > q0 + quads:
                raise ValueError("chunk {}: {{tensor {}, quad {}, quads {}}} does not tile tensor {} at quad {} (at most {} quads a chunk)".format(
                    c, ct, cq0, cquads, t, at, cq))
            if valid != min(4 * cquads, left) or valid < 1:
                raise ValueError("chunk {}: {} valid elements, {} expected".format(c, valid, min(4 * cquads, left)))
            at += cquads
            left -= valid
        if at != q0 + quads or left != 0:
            raise ValueError("tensor {}: its chunks cover {} of {} quads".format(t, at - q0, quads))
    if next_chunk != chunks.shape[0]:
        raise ValueError("{} chunks belong to no tensor".format(chunks.shape[0] - next_chunk))


def decode(ring, cursor: int, last_cursor: int = 0) -> Tuple[np.ndarray, int]:
    """(records [steps, T], dropped): the rows written between the counter values last_cursor and cursor, oldest first, and how many the
    ring no longer holds -- steplog.decode_ring for a ring of [capacity, T, 8] words (the counters are the step log's)."""
    return decode_ring(ring, cursor, last_cursor, RECORD_DTYPE, "T")


def split_tasks(records: np.ndarray, steps_per_task: int, n_tasks: int, dropped: int = 0) -> List[np.ndarray]:
    """steplog.split_tasks for [steps, T] rows: n_tasks runs of steps_per_task rows, by issue order."""
    S = int(steps_per_task)
    if S < 1 or dropped or len(records) != n_tasks * S:
        raise ValueError("layer log holds {} rows ({} dropped); {} tasks of {} steps were issued".format(len(records), dropped, n_tasks, S))
    return [records[k * S:(k + 1) * S] for k in range(n_tasks)]


def attribute(names: Sequence[str], step_records: np.ndarray, layer_records: np.ndarray) -> Optional[dict]:
    """Where a task's first non-finite step went wrong, by tensor; None when every step was finite.  step_records: the task's step-log
    records; layer_records: its [steps, T] rows.  {"step", "grad_nonfinite": (number of tensors whose gradient held a non-finite element
    at that step, the first NAMES_SHOWN of their names in arena order), "theta_nonfinite": the same for the parameters, "largest_grads":
    the LARGEST_SHOWN tensors with the largest grad_absmax in the last finite step before it as [(name, value)], None when step 0 was bad}.
    A non-finite value born in the backward pass marks only the tensors upstream of it; one born in the forward pass marks every tensor,
    and then largest_grads -- the trend before the divergence -- is the lead."""
    if layer_records.ndim != 2 or layer_records.shape[1] != len(names) or len(step_records) != len(layer_records):
        raise ValueError("{} step records, layer rows {}, {} names".format(len(step_records), layer_records.shape, len(names)))
    bad = np.flatnonzero(nonfinite_steps(step_records) | (layer_records["x_nonfinite"] > 0).any(axis=1) | (layer_records["y_nonfinite"] > 0).any(axis=1))
    if not bad.size:
        return None
    k = int(bad[0])
    out = {"step": k}
    for key, field in (("grad_nonfinite", "x_nonfinite"), ("theta_nonfinite", "y_nonfinite")):
        hit = np.flatnonzero(layer_records[field][k] > 0)
        out[key] = (int(hit.size), [names[i] for i in hit[:NAMES_SHOWN]])
    if k == 0:
        out["largest_grads"] = None
    else:
        amax = layer_records["x_absmax"][k - 1]
        order = np.argsort(-amax.astype(np.float64), kind="stable")[:LARGEST_SHOWN]
        out["largest_grads"] = [(names[i], float(amax[i])) for i in order]
    return out


def _mean_rows(rows) -> List[float]:
    return [float(v) for v in np.mean(np.asarray(rows, dtype=np.float64), axis=0)]


def _ratio_mean(num_rows, den_rows) -> List[Optional[float]]:
    """Per tensor the mean over tasks of num / den, None where a task's denominator is 0."""
    num, den = np.asarray(num_rows, dtype=np.float64), np.asarray(den_rows, dtype=np.float64)
    zero = (den == 0).any(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.mean(num / np.where(den == 0, 1.0, den), axis=0)
    return [None if z else float(v) for v, z in zip(mean, zero)]


def summarize(tasks: Sequence[Tuple[int, np.ndarray, np.ndarray, np.ndarray]], meta_iter: int = 0) -> dict:
    """One meta-iteration's row from [(task index, the task's step-log records, its [steps, T] layer rows, its [T] delta records)], the
    tasks of ONE rank; arrays of length T in arena order: grad_l2_first / grad_l2_last (mean over the tasks of the first / last step's
    gradient norm), grad_to_weight_last (mean over the tasks of lr * grad_l2 / theta_l2 at the last step, None where a task's theta_l2
    is 0), grad_absmax (maximum over tasks and steps), delta_l2 (mean over the tasks of ||theta_task - old||) and delta_rel (of
    delta_l2 / ||old||, None where ||old|| is 0)."""
    tasks = sorted(tasks, key=lambda t: t[0])
    row = {"meta_iter": int(meta_iter), "tasks": len(tasks)}
    filled = [t for t in tasks if len(t[2])]
    if not filled:
        row.update(grad_l2_first=None, grad_l2_last=None, grad_to_weight_last=None, grad_absmax=None, delta_l2=None, delta_rel=None)
        return row
    row["grad_l2_first"] = _mean_rows([lay["x_l2"][0] for _, _, lay, _ in filled])
    row["grad_l2_last"] = _mean_rows([lay["x_l2"][-1] for _, _, lay, _ in filled])
    row["grad_to_weight_last"] = _ratio_mean([np.float64(st["lr"][-1]) * lay["x_l2"][-1].astype(np.float64) for _, st, lay, _ in filled],
                                             [lay["y_l2"][-1] for _, _, lay, _ in filled])
    row["grad_absmax"] = [float(v) for v in np.max(np.stack([lay["x_absmax"].max(axis=0) for _, _, lay, _ in filled]), axis=0)]
    row["delta_l2"] = _mean_rows([d["x_l2"] for _, _, _, d in filled])
    row["delta_rel"] = _ratio_mean([d["x_l2"] for _, _, _, d in filled], [d["y_l2"] for _, _, _, d in filled])
    return row


def _json_value(v):
    return [_json_number(e) for e in v] if isinstance(v, list) else _json_number(v)


class LayerLogWriter:
    """<directory>/inner_loop_layers.jsonl: one summarize() row per line, appended and flushed as it comes; the tensor names of its arrays
    go once into <directory>/inner_loop_layers.names.json."""

    def __init__(self, directory: str, names: Sequence[str]):
        os.makedirs(directory, exist_ok=True)
        self.path = os.path.join(directory, "inner_loop_layers.jsonl")
        self.names_path = os.path.join(directory, "inner_loop_layers.names.json")
        with open(self.names_path, "w") as f:
            json.dump(list(names), f)
        self.f = open(self.path, "a")

    def add(self, row: dict):
        self.f.write(json.dumps({k: _json_value(v) for k, v in row.items()}) + "\n")
        self.f.flush()
