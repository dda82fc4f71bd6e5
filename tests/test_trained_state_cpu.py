"""The trained-like state of tests/trained_state.py: what the generator guarantees, and that a plain float32 implementation of the
step, started from it, stays well inside the tolerances of the step-parity tests (tests/test_step_trained_gpu.py) -- the condition
under which a device failure from this state is a device finding and not a property of the state."""
import numpy as np
import torch

import trained_state as TS
from oracle import efficientlab_ref as R
from test_step_gpu import _dc, _grad_tols

FP32_MARGIN = 0.25     # the float32 oracle must stay within this fraction of every tolerance (measured: 0.11 worst gradient tensor)


def _kind(name):
    return name.rsplit("/", 1)[1]


def test_generator_properties():
    variants = [R.OracleLearner(image_size=64, seed=0, dtype=torch.float32),
                R.OracleLearner(name="efficientnet-b3", image_size=64, seed=0, dtype=torch.float32, rsd=(2,), aspp=True, skip_decoding=True)]
    for O in variants:
        named = O.named_numpy()
        st = TS.trained_like(named)
        again = TS.trained_like(dict(reversed(list(named.items()))))           # deterministic, whatever the dict order
        assert list(st) == list(named)
        gammas = []
        for k, v in st.items():
            assert v.dtype == np.float32 and v.shape == named[k].shape, k
            assert np.array_equal(v, again[k]), k
            kind = _kind(k)
            if kind in ("kernel", "depthwise_kernel"):
                assert np.array_equal(v, named[k]), k
            elif kind == "gamma":
                assert np.all((np.abs(v) >= 0.5) & (np.abs(v) <= 1.5)), k
                gammas.append(v)
            elif kind in ("beta", "bias", "moving_mean"):
                assert np.any(v != 0), k
            else:
                assert kind == "moving_variance" and np.all((v >= 0.25) & (v <= 4.0)), k
        neg = np.mean(np.concatenate(gammas) < 0)
        assert 0.05 <= neg <= 0.20, neg
        other = TS.trained_like(named, seed=1)
        assert all(not np.array_equal(other[k], v) for k, v in st.items() if _kind(k) not in ("kernel", "depthwise_kernel"))
        # no two differently named tensors of equal shape are equal: exchanging any two of them changes the numbers
        by_shape = {}
        for k, v in st.items():
            by_shape.setdefault(v.shape, []).append(k)
        for names in by_shape.values():
            seen = {}
            for k in names:
                key = st[k].tobytes()
                assert key not in seen, (k, seen.get(key))
                seen[key] = k
        slots = TS.adam_slots({k: v for k, v in named.items() if k in O.params})
        assert list(slots) == list(O.params)
        for k, v in slots.items():
            assert v.dtype == np.float32 and v.shape == named[k].shape, k
            assert np.all((v >= np.float32(0.025 ** 2)) & (v <= np.float32(0.1 ** 2))), k


def test_float32_oracle_from_the_trained_like_state_stays_inside_the_step_tolerances():
    """One step of the 64x64 default network from the trained-like state, float64 oracle against float32 oracle, in the metric of
    test_step_gpu._compare_state.  Measured: worst gradient tensor at 0.11 of its tolerance, loss 5e-7 relative."""
    from mliis_amd.metaseg import synthetic_task
    H, idx = 64, [3, 1, 4, 0, 2, 3, 1, 1]
    x, y = synthetic_task(5, H, seed=1)
    out = {}
    for dt in (torch.float64, torch.float32):
        O = R.OracleLearner(image_size=H, seed=0, dtype=dt, lr=1e-3)
        O.load_named(TS.trained_like(O.named_numpy()))
        dc = _dc(O, len(idx), 5)
        lo, g, _ = R.inner_step(O.a, O.params, O.bn, torch.tensor(x[idx]).to(dt), torch.tensor(y[idx]).to(dt), 1e-3, dc)
        out[dt] = (lo, g, O)
    (lo, g, O), (lf, gf, Of) = out[torch.float64], out[torch.float32]
    assert abs(lf - lo) <= FP32_MARGIN * 1e-4 * max(1.0, abs(lo)), (lf, lo)
    tols = _grad_tols(g)
    ratios = {k: (gf[k].double() - g[k]).abs().max().item() / tols[k] for k in g}
    worst = max(ratios, key=ratios.get)
    print("float32 oracle: loss rel %.2e, worst gradient error / tolerance %.3f (%s)" % (abs(lf - lo) / abs(lo), ratios[worst], worst))
    assert ratios[worst] <= FP32_MARGIN, (worst, ratios[worst])
    for k in g:
        assert (Of.params[k].double() - O.params[k]).abs().max().item() <= FP32_MARGIN * 1e-5, k
    for k, (mm, mv) in O.bn.items():
        for ref, got in zip((mm, mv), Of.bn[k]):
            assert bool(((got.double() - ref).abs() <= FP32_MARGIN * (1e-5 + 1e-4 * ref.abs())).all()), k
