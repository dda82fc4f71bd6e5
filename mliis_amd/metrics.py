"""Host-side metrics of the evaluation surface: per-image IoU (reptile.py:526-549), Shaban-style counts
(reptile.py:552-566), CI95 (utils/util.py:133-136) and the EarlyStopper (hyperparam_search.py:24-68).
Values pinned by tests/golden/host_logic.json."""
import operator
from typing import Optional, Sequence

import numpy as np


def iou(prediction: np.ndarray, label: np.ndarray, epsilon: float = 1e-7, class_of_interest_channel: Optional[int] = 1,
        round_labels: bool = True) -> float:
    prediction, label = np.asarray(prediction), np.asarray(label)
    if prediction.ndim > 3:
        raise ValueError("Function is intended for single image masks, not batches.")
    if prediction.shape != label.shape:
        raise ValueError("prediction shape and label shape must be equal but are: {} and {} respectively.".format(
            prediction.shape, label.shape))
    if class_of_interest_channel is not None:
        prediction, label = prediction[..., class_of_interest_channel], label[..., class_of_interest_channel]
    p = np.round(prediction).astype(bool)
    l = (np.round(label) if round_labels else label).astype(bool)
    return (np.count_nonzero(p & l) + epsilon) / (np.count_nonzero(p | l) + epsilon)


def iou_from_counts(intersection, union, epsilon: float = 1e-7) -> float:
    """iou() from the two pixel counts it ends in (ops.mask_iou_counts: counts[n][0], counts[n][1]): the same float64 expression, so
    the two agree to the last bit."""
    return (int(intersection) + epsilon) / (int(union) + epsilon)


def unpack_mask(words, H: int, W: int) -> np.ndarray:
    """bool [..., H, W] from the bit-packed masks of ops.mask_pack (host int64 / uint64 words [..., ceil(H W / 64)]): bit 0 of a word is
    its first pixel (little-endian bit order, linear over the image); the first H W bits are taken, set bits beyond them ignored."""
    w = np.ascontiguousarray(words)
    if w.dtype not in (np.dtype(np.int64), np.dtype(np.uint64)):
        raise ValueError("unpack_mask: expected int64 / uint64 words, got {}".format(w.dtype))
    H, W = int(H), int(W)
    if w.ndim < 1 or w.shape[-1] != (H * W + 63) // 64:
        raise ValueError("unpack_mask: {} words per image for {} x {} pixels".format(w.shape[-1] if w.ndim else 0, H, W))
    bytes_ = w.astype("<u8", copy=False).view(np.uint8).reshape(w.shape[:-1] + (w.shape[-1] * 8,))
    bits = np.unpackbits(bytes_, axis=-1, bitorder="little")[..., :H * W]
    return bits.astype(bool).reshape(w.shape[:-1] + (H, W))


def measure(y_in, pred_in, thresh: float = 0.5):
    y, p = np.asarray(y_in) > thresh, np.asarray(pred_in) > thresh
    return (int((y & p).sum()), int((~y & ~p).sum()), int((~y & p).sum()), int((y & ~p).sum()))


def iou_img(tp, fp, fn) -> float:
    return tp / float(max(tp + fp + fn, 1))


def ci95(a: Sequence[float]) -> float:
    a = np.asarray(a, dtype=np.float64)
    return float(1.96 * a.std() / np.sqrt(len(a)))


class EarlyStopper:
    def __init__(self, patience: int = 10, metric_should_increase: bool = True, min_steps: int = 0):
        self.patience, self.min_steps = patience, min_steps
        self._better = operator.gt if metric_should_increase else operator.lt
        self._best_metric = None
        self._best_num_steps = min_steps if min_steps > 0 else None
        self.num_evals_without_improving = 0

    def continue_training(self, metric, total_steps_taken) -> bool:
        if total_steps_taken <= self.min_steps:
            self._best_metric = metric
            return True
        if self._best_metric is None or self._better(metric, self._best_metric):
            self.num_evals_without_improving = 0
            self._best_metric, self._best_num_steps = metric, total_steps_taken
            return True
        self.num_evals_without_improving += 1
        return self.num_evals_without_improving <= self.patience

    def best_metric(self):
        return self._best_metric

    def best_num_steps(self):
        return self._best_num_steps


# ------------------------------------------------------------------------------------------------ the threshold sweep (host numpy only)
HIST_BINS = 256   # bins per label class of ops.prob_histogram (mliis_prob_hist_bins)


def _hist(hist) -> np.ndarray:
    h = np.asarray(hist)
    if h.ndim < 2 or h.shape[-2:] != (2, HIST_BINS) or h.dtype.kind not in "iu":
        raise ValueError("expected integer histograms [..., 2, {}], got {} {}".format(HIST_BINS, h.shape, h.dtype))
    return h.astype(np.int64)


def counts_from_histogram(hist) -> np.ndarray:
    """int64 [..., 256, 4] from the histograms of ops.prob_histogram (int [..., 2, 256]: label class, bin): row k = {|P_k & L|, |P_k | L|,
    |P_k|, |L|} with P_k = (p1 > k/256) = (bin >= k) for k = 1..255 -- row 128 is ops.mask_iou_counts' row bit for bit -- and row 0 the
    "everything predicted" row (bin >= 0).  Exact: integer suffix sums."""
    h = _hist(hist)
    tail = np.cumsum(h[..., ::-1], axis=-1)[..., ::-1]        # tail[..., c, k] = pixels of class c in bins >= k
    inter, pred = tail[..., 1, :], tail[..., 0, :] + tail[..., 1, :]
    lab = np.broadcast_to(h[..., 1, :].sum(axis=-1)[..., None], inter.shape)
    return np.stack([inter, pred + lab - inter, pred, lab], axis=-1)


def iou_curve(hist, epsilon: float = 1e-7) -> np.ndarray:
    """float64 [..., 256]: iou_from_counts' expression on every row of counts_from_histogram (entry 128 = the IoU the project reports)."""
    c = counts_from_histogram(hist)
    return (c[..., 0] + epsilon) / (c[..., 1] + epsilon)


def reliability(hist) -> dict:
    """The reliability table of histograms pooled over their leading axes: per bin the pixel count, the foreground share (None for an
    empty bin) and the bin centre (b + 0.5) / 256 taken as its confidence, and the expected calibration error
    sum_b count_b / total |share_b - centre_b|."""
    h = _hist(hist).reshape(-1, 2, HIST_BINS).sum(axis=0)
    count = h[0] + h[1]
    centre = (np.arange(HIST_BINS) + 0.5) / HIST_BINS
    total = int(count.sum())
    filled = count > 0
    share = np.full(HIST_BINS, np.nan)
    share[filled] = h[1][filled] / count[filled]
    ece = float((count[filled] / total * np.abs(share[filled] - centre[filled])).sum()) if total else float("nan")
    return {"count": [int(c) for c in count], "foreground_share": [float(s) if f else None for s, f in zip(share, filled)],
            "confidence": [float(c) for c in centre], "pixels": total, "ece": ece}


def mean_curve(curves) -> np.ndarray:
    """float64 [256]: np.nanmean over the rows of curves [n, 256].  Entry 128 is summed as the 1-D array the evaluation loops average, so
    it is, to the last bit, float(np.nanmean([...])) of the rows' IoUs at 0.5 (the printed means); the other entries are one reduction
    over the rows, which may differ from that in the last bit once there are eight rows or more (numpy sums a contiguous vector pairwise)."""
    import warnings
    c = np.asarray(curves, dtype=np.float64).reshape(-1, HIST_BINS)
    half = HIST_BINS // 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        m = np.nanmean(c, axis=0) if len(c) else np.full(HIST_BINS, np.nan)
        m[half] = float(np.nanmean(np.ascontiguousarray(c[:, half]))) if len(c) else np.nan
    return m


def best_threshold_index(curve) -> int:
    """argmax over k = 1..255 of curve [256]; among equal maxima the k nearest 128 (threshold 0.5), of two equally near the smaller."""
    c = np.asarray(curve, dtype=np.float64)[1:HIST_BINS]
    c = np.where(np.isnan(c), -np.inf, c)
    ks = np.flatnonzero(c == c.max()) + 1
    return int(min(ks, key=lambda k: (abs(int(k) - HIST_BINS // 2), int(k))))


def threshold_summary(curves) -> dict:
    """From IoU curves [n, 256] (iou_curve rows, or means of them): the thresholds k/256 for k = 1..255, their mean curve (mean_curve),
    the best threshold (best_threshold_index: ties go to the one nearest 0.5) and the mean IoU at 0.5 and at the best."""
    m = mean_curve(curves)
    k = best_threshold_index(m)
    return {"thresholds": [i / HIST_BINS for i in range(1, HIST_BINS)], "mean_iou": [float(v) for v in m[1:]],
            "iou_at_0.5": float(m[HIST_BINS // 2]), "best_threshold": k / HIST_BINS, "iou_at_best": float(m[k])}


class ThresholdSweep:
    """The sink of Gecko(threshold_sweep=...): called once per evaluated task with (task name, per-image IoU curves [n, 256], per-image
    histograms [n, 2, 256]); evaluate_gecko announces every evaluation pass with begin_pass().  summary() aggregates as the printed mean
    does -- per task the mean over its images, per pass the mean over its tasks, then the mean over the passes -- so its "iou_at_0.5" is
    the float evaluate_gecko returns."""

    def __init__(self):
        self.passes = []                                               # per pass: [(task name, mean curve of its images)]
        self.pooled = np.zeros((2, HIST_BINS), dtype=np.int64)         # all pixels seen

    def begin_pass(self, sample_num=None):
        self.passes.append([])

    def __call__(self, task_name, curves, hists):
        if not self.passes:
            self.begin_pass()
        self.passes[-1].append((task_name, mean_curve(curves)))
        self.pooled += _hist(hists).reshape(-1, 2, HIST_BINS).sum(axis=0)

    def pass_curves(self) -> np.ndarray:
        """float64 [passes, 256]: every pass's mean over its tasks."""
        return np.stack([mean_curve([c for _, c in p]) for p in self.passes if p]) if any(self.passes) else np.zeros((0, HIST_BINS))

    def mean(self) -> np.ndarray:
        return mean_curve(self.pass_curves())

    def summary(self) -> dict:
        out = threshold_summary(self.pass_curves())
        tasks = {}
        for p in self.passes:
            for name, c in p:
                tasks.setdefault(name, []).append(c)
        out["tasks"] = {}
        for name, cs in tasks.items():
            m = mean_curve(cs)
            k = best_threshold_index(m)
            out["tasks"][name] = {"best_threshold": k / HIST_BINS, "iou_at_best": float(m[k]), "iou_at_0.5": float(m[HIST_BINS // 2])}
        rel = reliability(self.pooled)
        out["ece"] = rel["ece"]
        out["reliability"] = rel
        return out
