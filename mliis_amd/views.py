"""The views of flip test-time augmentation at evaluation (host only: names, their order, what they mirror).

A view set is any subset of VIEWS without repeats; the identity view is always part of the merge and has no name; the empty set means
the feature is off.  canonical() puts a set into the order of VIEWS, so a result never depends on the order the views were asked for."""
from __future__ import annotations

from typing import Iterable, Tuple

# name -> (rows mirrored: h -> H-1-h, columns mirrored: w -> W-1-w); hflip is np.fliplr of an [H,W,C] image
FLIPS = {"hflip": (False, True), "vflip": (True, False), "hvflip": (True, True)}
VIEWS = ("hflip", "vflip", "hvflip")


def canonical(views: Iterable[str]) -> Tuple[str, ...]:
    """The view set as a tuple in the order of VIEWS; ValueError for an unknown name or a repeat.  None and () give ()."""
    if views is None:
        return ()
    if isinstance(views, str):
        views = (views,)
    views = list(views)
    for v in views:
        if v not in FLIPS:
            raise ValueError("unknown test-time-augmentation view {!r}: the views are {}".format(v, ", ".join(VIEWS)))
    if len(set(views)) != len(views):
        raise ValueError("a test-time-augmentation view is given more than once: {}".format(views))
    return tuple(v for v in VIEWS if v in views)


def accepts_views(fn) -> bool:
    """Whether the callable takes the keyword `views` (a learner method of the device Learner does; the CPU oracle's do not)."""
    import inspect
    try:
        params = inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False
    return "views" in params   # (a **kwargs that swallows it is no support: the views would be dropped silently)


SCORING_METHODS = ("predict_resident", "score_resident", "mask_resident", "histogram_resident")


def require_views_support(learners, views) -> None:
    """ValueError unless every learner's scoring methods (those it has; predict_resident at least) take views=."""
    if not views:
        return
    for ln in learners:
        fns = [getattr(ln, m, None) for m in SCORING_METHODS]
        if not callable(fns[0]) or not all(accepts_views(f) for f in fns if callable(f)):
            raise ValueError("eval_views={} needs a learner (and lanes) whose scoring methods take views= (the device Learner; the CPU "
                             "oracle has none): {}".format(tuple(views), type(ln).__name__))
