"""A deterministic trained-like network state for the step-parity tests (a plain module: tests import it, nothing here is collected).

oracle.efficientlab_ref.init_state is ONE point of parameter space: every batch-norm gamma is 1 and beta 0, every bias 0, every moving
mean 0 and moving variance 1.  From there two parameter sets of equal length are indistinguishable (gamma of the depthwise batch norm
where the expand batch norm's is meant, the beta of another layer with the same channel count, a dropped conv bias, another layer's
moving statistics in the inference plan): a step that wires them wrongly computes the same numbers as the correct one.
trained_like() replaces exactly those tensors by values no two of which agree; the kernels (conv, depthwise, squeeze-excite) stay.

Every tensor is drawn from np.random.default_rng([seed, crc32(name)]): independent of the other tensors and of dict order, so a
network variant (other decoder, other encoder) gives the tensors it shares with another variant the same values.
"""
from __future__ import annotations

import zlib
from typing import Dict

import numpy as np

GAMMA_NEGATIVE_BELOW = 0.125     # a gamma entry is negated where a second uniform draw falls below this


def _rng(seed: int, name: str):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode())])


def trained_like(named: Dict[str, np.ndarray], seed: int = 0) -> Dict[str, np.ndarray]:
    """`named`: what OracleLearner.named_numpy() returns.  float32 arrays of the same shapes:
        */gamma            U(0.5, 1.5), negated where a second uniform draw is < 0.125 (a negative gamma is legal, and the case that
                           catches an rstd * gamma folded through an absolute value or a square root)
        */beta             N(0, 0.5)
        */bias             N(0, 0.2)
        */moving_mean      N(0, 0.5)
        */moving_variance  U(0.25, 4)
        anything else      unchanged"""
    out = {}
    for name, v in named.items():
        v = np.asarray(v)
        g = _rng(seed, name)
        if name.endswith("/gamma"):
            mag = g.uniform(0.5, 1.5, v.shape)
            a = np.where(g.uniform(0.0, 1.0, v.shape) < GAMMA_NEGATIVE_BELOW, -mag, mag)
        elif name.endswith("/beta") or name.endswith("/moving_mean"):
            a = g.normal(0.0, 0.5, v.shape)
        elif name.endswith("/bias"):
            a = g.normal(0.0, 0.2, v.shape)
        elif name.endswith("/moving_variance"):
            a = g.uniform(0.25, 4.0, v.shape)
        else:
            a = v
        out[name] = np.array(a, dtype=np.float32)
    return out


def adam_slots(named_trainables: Dict[str, np.ndarray], seed: int = 1) -> Dict[str, np.ndarray]:
    """A warm Adam second moment per trainable: (0.05 * U(0.5, 2))**2 per element, float32 (gradient magnitudes of 0.025 .. 0.1)."""
    return {name: np.array((0.05 * _rng(seed, name).uniform(0.5, 2.0, np.shape(v))) ** 2, dtype=np.float32)
            for name, v in named_trainables.items()}


def load_device(L, state: Dict[str, np.ndarray], extra: Dict[str, np.ndarray] = None):
    """`state` into the device learner; what it then holds is `state` bit for bit (trainables and moving statistics: the load path is
    part of what is tested).  `extra`: further entries (Adam slots and step entries, which the oracle takes through inner_step's
    adam_state)."""
    L.load_named({**state, **(extra or {})}, strict=False)
    got = L.named_numpy()
    for k, v in state.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape, k
        assert np.array_equal(got[k].view(np.uint32), v.view(np.uint32)), k


def load_both(O, L, state: Dict[str, np.ndarray], extra: Dict[str, np.ndarray] = None):
    """The same float32 numbers into the oracle (every variable it has must be in `state`) and the device learner."""
    O.load_named(state)
    load_device(L, state, extra)
