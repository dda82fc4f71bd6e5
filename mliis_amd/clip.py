"""The inner loop's gradient clipping, host side: the modes and record layout of csrc/clip.hip (include/mliis_clip.h), the decoder of the
device ring and the per-meta-iteration summary.  numpy only -- nothing here needs a device.

A learner built with grad_clip=("norm", C) or ("ratio", LAMBDA, EPS) bounds the loss gradient between its backward pass and its optimizer
launch, in every training step, and writes one row of R records (R = 1 by global norm, R = T trainable tensors per tensor) per step into a
ring of clip_log rows (Learner.read_clip_log copies ring and cursor back and calls decode()).  The chunk tables are the per-tensor log's
(layerlog.chunk_table / validate_table with this library's chunk size).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np

from .steplog import decode_ring

RECORD_WORDS = 8
RECORD_DTYPE = np.dtype([("g_l2", "<f4"), ("ref", "<f4"), ("scale", "<f4"), ("nonfinite", "<u4"), ("flags", "<u4"), ("zero", "<u4", (3,))])
assert RECORD_DTYPE.itemsize == 4 * RECORD_WORDS
MODES = {"norm": 0, "ratio": 1}
CLIPPED, BYPASSED = 1, 2          # bits of "flags"
DEFAULT_RATIO_EPS = 1e-3


def parse(grad_clip) -> Optional[Tuple[str, float, float]]:
    """None | ("norm", C) | ("ratio", LAMBDA[, EPS]) -> None | (mode, threshold, eps); ValueError on anything else, or a value that is not
    finite and positive."""
    if grad_clip is None:
        return None
    try:
        mode, values = grad_clip[0], [float(v) for v in grad_clip[1:]]
    except (TypeError, ValueError, IndexError):
        raise ValueError("grad_clip must be None, ('norm', C) or ('ratio', LAMBDA, EPS), got {!r}".format(grad_clip)) from None
    if mode not in MODES or not 1 <= len(values) <= (1 if mode == "norm" else 2):
        raise ValueError("grad_clip must be None, ('norm', C) or ('ratio', LAMBDA, EPS), got {!r}".format(grad_clip))
    if mode == "ratio" and len(values) == 1:
        values.append(DEFAULT_RATIO_EPS)
    if not all(math.isfinite(v) and v > 0 for v in values):
        raise ValueError("grad_clip {!r}: thresholds and eps are finite and positive".format(grad_clip))
    return mode, values[0], (values[1] if mode == "ratio" else DEFAULT_RATIO_EPS)


def decode(ring, cursor: int, last_cursor: int = 0) -> Tuple[np.ndarray, int]:
    """(records [steps, R], dropped): the rows written between the counter values last_cursor and cursor, oldest first, and how many of
    them the ring no longer holds -- steplog.decode_ring for a ring of [capacity, R, 8] words (the counters are taken modulo 2^32 like the
    device's)."""
    return decode_ring(ring, cursor, last_cursor, RECORD_DTYPE, "R")


def clipped_steps(records: np.ndarray) -> np.ndarray:
    """bool per step: some record of the row has the clipped flag."""
    return ((records["flags"] & CLIPPED) != 0).any(axis=1)


def bypassed_steps(records: np.ndarray) -> np.ndarray:
    """bool per step: the gradient held a non-finite element and was left as it was."""
    return ((records["flags"] & BYPASSED) != 0).any(axis=1)


def _row_norm(rows: np.ndarray) -> float:
    """The pre-clip norm of one step's whole gradient from its R records (R = 1: the record's own)."""
    return float(np.sqrt(np.sum(rows["g_l2"].astype(np.float64) ** 2)))


def summarize(task_records: Sequence[Tuple[int, np.ndarray]]) -> dict:
    """The clip's keys of one meta-iteration's inner_loop.jsonl line from [(task index, that task's [steps, R] rows)], the tasks of ONE
    rank: clip_frac (share of the steps in which some scale was below the bound), clip_scale_min (the smallest scale applied, 1.0 when
    none was), grad_l2_preclip_first / grad_l2_preclip_last (mean over the tasks of the first / last step's pre-clip norm of the whole
    gradient, over its finite elements) and clip_bypassed (steps whose gradient held a non-finite element and was left as it was).  Plain
    Python numbers; None where there is no step."""
    filled = [r for _, r in sorted(task_records, key=lambda tr: tr[0]) if len(r)]
    steps = sum(len(r) for r in filled)
    if not steps:
        return dict(clip_frac=None, clip_scale_min=None, grad_l2_preclip_first=None, grad_l2_preclip_last=None, clip_bypassed=0)
    return dict(clip_frac=float(sum(int(clipped_steps(r).sum()) for r in filled)) / steps,
                clip_scale_min=float(min(float(r["scale"].min()) for r in filled)),
                grad_l2_preclip_first=float(np.mean([_row_norm(r[0]) for r in filled])),
                grad_l2_preclip_last=float(np.mean([_row_norm(r[-1]) for r in filled])),
                clip_bypassed=int(sum(int(bypassed_steps(r).sum()) for r in filled)))
