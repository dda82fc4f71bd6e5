"""Inner-step parity from a trained-like state: mliis_amd.Learner (HIP, fp32) vs the float64 CPU oracle, both loaded with
tests/trained_state.py -- batch-norm gamma in +-[0.5, 1.5], beta / conv bias / squeeze-excite bias / final-layer bias non-zero, moving
statistics away from (0, 1), and (case G) warm Adam slots.  Every other step-parity test starts from oracle.init_state, where gamma
= 1, beta = bias = 0 and moving = (0, 1) make two parameter sets of equal length indistinguishable: a launch that is handed bn1's
gamma where bn0's is meant, a dropped conv bias or another layer's moving statistics computes the same numbers there.  Here it does not.

Tolerances: those of tests/test_step_gpu.py, unchanged (loss 1e-4 first step / 1e-3 later; gradients, parameters and moving statistics
through _compare_state; inference logits 2e-3 of the logit scale; masks equal outside a 1e-3 margin).

The state keeps a plain fp32 implementation well inside them (tests/test_trained_state_cpu.py asserts the first line):
  float32 oracle vs float64 oracle on the CPU, worst gradient error / tolerance
    64x64 B0 default, one step                        0.11   (blocks_3/se/conv2d/bias; loss 4.7e-7 relative)
    64x64, three steps: B0 default / B0 ASPP + skip decoding / B3 skip decoding RSD(2,) / B0 ASPP only
                                                      0.10 / 0.11 / 0.10 / 0.07
    128x128 B0 default                                0.09
    later-step loss <= 2e-6 relative, parameters after three steps <= 7e-7, inference logits <= 6e-6 of scale, >= 99.7 % of the
    pixels outside the mask margin
    case G: worst element at 0.18 of the parameter bound (0.30 with 2**-23 in place of 2**-22); largest update 2.8e-3
  device (MI355X) vs float64 oracle, worst gradient error / tolerance (MLIIS_TEST_VERBOSE=1 ... -s prints them)
    A default plan                                    0.054  (blocks_3/se/conv2d/kernel; logits 4.3e-6 of scale inference, 2.4e-5 training)
    B op by op                                        0.038  (blocks_0/tpu_batch_normalization/beta)
    C project BN on load, fuse_head False / True      0.072 / 0.072  (blocks_2/tpu_batch_normalization/gamma)
    D split products / fp32-native at 128x128         0.064 / 0.069
    E ASPP + skip decoding + RSD(2, 4) / ASPP only    0.087 / 0.073  (logits <= 2.3e-5 of scale in either mode)
    F B3 skip decoding RSD(2,)                        0.136  (blocks_1/se/conv2d/bias; logits <= 3.5e-5 of scale)
    G adam                                            0.047; worst parameter error / bound 0.185 (decode_skip_connections_1/batch_normalization/beta)
    at least 99.5 % of the pixels outside the mask margin in every case
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import trained_state as TS  # noqa: E402
from oracle import efficientlab_ref as R  # noqa: E402
from test_step_gpu import _compare_grads, _compare_state, _dc, _grad_tols, _mask_check, _need_gpu, _task  # noqa: E402

IDX = [3, 1, 4, 0, 2, 3, 1, 1]


def _oracle(H, **variant):
    """(float64 oracle loaded with the trained-like state, the state)."""
    O = R.OracleLearner(image_size=H, seed=0, dtype=torch.float64, lr=1e-3, **variant)
    state = TS.trained_like(O.named_numpy())
    O.load_named(state)
    return O, state


def _learner(H, state, variant=None, extra=None, **kw):
    from mliis_amd.learner import Learner
    v = dict(variant or {})
    L = Learner(feature_extractor_name=v.get("name", "efficientnet-b0"), image_size=H, seed=100, rsd=v.get("rsd", (2, 4)),
                spatial_pyramid_pooling=v.get("aspp", False), skip_decoding=v.get("skip_decoding", False), **kw)
    TS.load_device(L, state, extra)
    return L


def _ref_step(H, idx, task_seed, dc_seed):
    O, state = _oracle(H)
    x, y = _task(5, H, task_seed)
    dc = _dc(O, len(idx), dc_seed)
    lo, gO, _ = R.inner_step(O.a, O.params, O.bn, torch.tensor(x[idx]).double(), torch.tensor(y[idx]).double(), 1e-3, dc)
    return dict(O=O, state=state, x=x, y=y, dc=dc, lo=lo, gO=gO)


@functools.lru_cache(maxsize=None)
def _ref64():
    """The first step of the default network at 64x64 on the oracle: computed once, shared by cases A, B and C, never modified."""
    return _ref_step(64, IDX, 1, 5)


def _first_step(L, ref, idx, tag):
    L.load_task(ref["x"], ref["y"])
    L.inner_step(idx, dc_scales=ref["dc"])
    ll, lo = L.loss_value(), ref["lo"]
    assert abs(ll - lo) <= 1e-4 * max(1.0, abs(lo)), (tag, ll, lo)
    _compare_state(ref["O"], L, ref["gO"], tag)


def _inference(O, L, x, tag, modes=(False, True)):
    xd = torch.tensor(x).double()
    for training in modes:
        with torch.no_grad():
            lgO, _ = R.forward(O.a, O.params, O.bn, xd, training)
        pL, lgL = L.predict(x, training=training, return_logits=True)
        scale = lgO.abs().max().item()
        err = (lgL.cpu().double() - lgO).abs().max().item()
        if os.environ.get("MLIIS_TEST_VERBOSE"):
            print("%s, %s mode: logit error %.2e of scale (bound 2e-3)" % (tag, "training" if training else "inference", err / scale))
        assert err <= 2e-3 * scale, (tag, training, err, scale)
        _mask_check(pL, lgO, 1e-3, "%s, %s-mode masks" % (tag, "training" if training else "inference"), min_outside=0.99)


def _three_steps_and_inference(variant, tag, idx, task_seed):
    """Steps eager / captured / replayed with injected drop-connect (and ASPP) masks, _compare_state after the first, then predict."""
    H = 64
    O, state = _oracle(H, **variant)
    L = _learner(H, state, variant, use_graph=True)
    assert [p.name for p in L.arena.trainable] == list(O.params)
    x, y = _task(5, H, task_seed)
    L.load_task(x, y)
    xb, yb = torch.tensor(x[idx]).double(), torch.tensor(y[idx]).double()
    N, d, h = len(idx), O.a["dec_c"], H // 16
    g = np.random.default_rng(9)
    for step in range(3):
        dc = _dc(O, N, 20 + step)
        kw = {}
        if variant.get("aspp"):
            kw["aspp_masks"] = [torch.tensor(2.0 * (g.random(s) < 0.5)) for s in ((N, h, h, d), (N, h, h, d), (N, 1, 1, d), (N, h, h, d))]
        lo, gO, _ = R.inner_step(O.a, O.params, O.bn, xb, yb, 1e-3, dc, **kw)
        L.inner_step(idx, dc_scales=dc, **kw)
        ll = L.loss_value()
        assert abs(ll - lo) <= (1e-4 if step == 0 else 1e-3) * max(1.0, abs(lo)), (tag, step, ll, lo)
        if step == 0:
            _compare_state(O, L, gO, tag)
    assert L.plans[N].graph is not None
    _inference(O, L, x, tag)
    L.close()


def test_a_default_plan_three_steps_and_inference():
    """The plan every run takes: three steps (eager, captured, replayed), then predict in inference mode -- the first test in which the
    moving statistics the device reads are not (0, 1) -- and in training mode."""
    _need_gpu()
    ref = _ref64()
    L = _learner(64, ref["state"], use_graph=True)
    _first_step(L, ref, IDX, "A default plan")
    O = R.OracleLearner(image_size=64, seed=0, dtype=torch.float64, lr=1e-3)
    O.import_all(ref["O"].export_all())                # (the shared first step stays as it is)
    xb, yb = torch.tensor(ref["x"][IDX]).double(), torch.tensor(ref["y"][IDX]).double()
    for step in (1, 2):
        dc = _dc(O, len(IDX), 5 + step)
        lo = O.inner_step(xb, yb, dc_scales=dc)
        L.inner_step(IDX, dc_scales=dc)
        ll = L.loss_value()
        assert abs(ll - lo) <= 1e-3 * max(1.0, abs(lo)), (step, ll, lo)
    assert L.plans[8].graph is not None
    _inference(O, L, ref["x"], "A default plan")
    L.close()


def test_b_op_by_op_depthwise_path():
    _need_gpu()
    ref = _ref64()
    L = _learner(64, ref["state"], use_graph=False, small_fused=False, dw_march=False)
    _first_step(L, ref, IDX, "B op by op")
    assert not any(B["small"] or B["march"] for B in L.plans[8].blocks)
    L.close()


@pytest.mark.parametrize("fuse_head", [False, True])
def test_c_project_batch_norm_on_load(fuse_head):
    """Learner(fuse_bn2=True): mliis_conv2d_fwd_bnin applies the PREVIOUS block's project gamma / beta / drop-connect / skip on load."""
    _need_gpu()
    ref = _ref64()
    L = _learner(64, ref["state"], use_graph=False, fuse_bn2=True, fuse_head=fuse_head)
    _first_step(L, ref, IDX, "C project BN on load, fuse_head=%s" % fuse_head)
    assert any(L.plans[8].bn2_deferred)
    L.close()


def test_d_split_product_decoder_at_128():
    """128x128, N = 8: the smallest size whose 32x32 decoder maps reach _Passes.X3_MIN_ROWS rows.  Non-zero conv biases and an RSD border
    bias beside a bias term reach mliis_conv2d_fwd_x3; then the native fp32 instruction on the same state, same tolerances."""
    _need_gpu()
    H, idx = 128, [0, 1, 2, 3, 4, 0, 1, 2]
    ref = _ref_step(H, idx, 0, 3)
    L = _learner(H, ref["state"], use_graph=False)
    assert L.x3 is not None and len(L.x3.rows) == 8     # two modules x {dilated branch, fuse conv} x {fwd, bwd}
    _first_step(L, ref, idx, "D split products")
    took = []
    for nm, D in zip(L.n_rsd, L.plans[8].rsd):
        rows = D["cat"].shape[0] * D["cat"].shape[1] * D["cat"].shape[2]
        assert L._x3_takes(nm[1][0], D["cat"]) == L._x3_takes(nm[2][0], D["pyr"]) == (rows >= L.X3_MIN_ROWS)
        took.append(L._x3_takes(nm[1][0], D["cat"]))
    assert sorted(took) == [False, True]               # the 32x32 level takes them, the 8x8 level does not
    assert not L._x3_takes(L.n_blocks[3]["w_proj"], L.plans[8].rsd[took.index(True)]["cat"])
    L.close()
    L0 = _learner(H, ref["state"], use_graph=False, matmul_precision="fp32-native")
    assert L0.x3 is None
    _first_step(L0, ref, idx, "D fp32-native")
    L0.close()


@pytest.mark.parametrize("variant", [dict(rsd=(2, 4), aspp=True, skip_decoding=True), dict(rsd=(), aspp=True)],
                         ids=["aspp-skipdec-rsd24", "aspp-only"])
def test_e_optional_decoders(variant):
    _need_gpu()
    _three_steps_and_inference(variant, "E " + "/".join("%s=%s" % kv for kv in variant.items()), [3, 1, 4, 0, 2, 3], 3)


def test_predict_in_training_mode_reads_no_mask_buffer():
    """predict(training=True) means batch statistics; the drop-connect scales and the dropout masks (ASPP, final layer) belong to a
    training step.  Case E found predict reading the ASPP mask buffers of a plan no step had written (logit error 40 at a scale of 56).
    A step on the plan that predict() shares leaves drawn masks in the buffers; the logits must not change, bit for bit, when every
    one of them is then overwritten with NaN."""
    _need_gpu()
    H, idx = 64, [3, 1, 4, 0, 2]
    _, state = _oracle(H, aspp=True)
    L = _learner(H, state, dict(aspp=True), use_graph=False, final_layer_dropout_rate=0.5)
    x, y = _task(5, H, 3)
    L.load_task(x, y)
    L.inner_step(idx)                                   # (draws every mask of the N = 5 plan)
    P = L.plans[5]
    assert P.drop_mask is not None and (P.drop_mask == 0).any() and all((m == 0).any() for m in P.aspp["masks"])
    _, first = L.predict(x, training=True, return_logits=True)
    for buf in [P.drop_mask, P.dc_all] + P.aspp["masks"]:
        buf.fill_(float("nan"))
    _, second = L.predict(x, training=True, return_logits=True)
    assert not torch.isnan(second).any() and torch.equal(first, second)
    L.close()


def test_f_efficientnet_b3():
    """Blocks without an expand conv, the noexpand_dw_bwd path, the never-executed blocks (their state must stay as loaded)."""
    _need_gpu()
    _three_steps_and_inference(dict(name="efficientnet-b3", skip_decoding=True, rsd=(2,)), "F B3", [3, 1, 4, 0, 2, 3], 3)


def test_g_adam_from_a_warm_optimizer_state():
    """Adam(beta1 = 0) with second moments v > 0 and seven steps behind it.  From a cold start the comparison can only be statistical
    (test_step_gpu.test_dropout_adam_and_b3_variants); from here it is a bound: the update lr * c * g / (sqrt(v') + eps), v' = 0.999 v
    + 0.001 g^2, c = sqrt(1 - 0.999^8), has a derivative in g of at most lr * c / sqrt(0.999 v) in magnitude, so per element
    |theta_dev - theta_ref| <= lr * c * tol_g / sqrt(0.999 v) + 2^-22 |theta| with tol_g the tensor's gradient tolerance.  The largest
    update is 2.8e-3: a wrong offset into v or a wrong step count shows."""
    _need_gpu()
    from mliis_amd.checkpoint import adam_step_entries
    H, lr, T0 = 64, 1e-3, 7
    O, state = _oracle(H)
    v = TS.adam_slots({k: state[k] for k in O.params})
    extra = {k + "/Adam_1": a for k, a in v.items()}
    extra.update(adam_step_entries(T0, 0.999))
    L = _learner(H, state, extra=extra, optimizer="adam", use_graph=True, drop_connect=False)
    assert L.adam_t.item() == T0
    got = L.named_numpy()
    assert all(np.array_equal(got[k], a) for k, a in extra.items() if k.endswith("/Adam_1"))
    x, y = _task(5, H, 1)
    L.load_task(x, y)
    xb, yb = torch.tensor(x[IDX]).double(), torch.tensor(y[IDX]).double()
    st = {"t": T0, "v": {k: torch.tensor(a).double() for k, a in v.items()}}
    lo, gO, _ = R.inner_step(O.a, O.params, O.bn, xb, yb, lr, None, None, adam_state=st)
    L.inner_step(IDX)
    ll = L.loss_value()
    assert abs(ll - lo) <= 1e-4 * max(1.0, abs(lo)), (ll, lo)
    assert L.adam_t.item() == T0 + 1
    _compare_grads(L, gO, "G adam")
    tols, c = _grad_tols(gO), math.sqrt(1.0 - 0.999 ** (T0 + 1))
    th = L.arena.export_trainable_packed().cpu().double()
    off, ratios = 0, []
    for p in L.arena.trainable:
        ref = O.params[p.name].reshape(-1)
        bound = lr * c * tols[p.name] / torch.sqrt(0.999 * torch.tensor(v[p.name]).double().reshape(-1)) + 2.0 ** -22 * ref.abs()
        ratios.append((((th[off:off + p.size] - ref).abs() / bound).max().item(), p.name))
        off += p.size
    if os.environ.get("MLIIS_TEST_VERBOSE"):
        print("G adam: worst parameter error / bound %.3f (%s)" % max(ratios))
    for ratio, name in ratios:
        assert ratio <= 1.0, (name, ratio)
    lo = R.inner_step(O.a, O.params, O.bn, xb, yb, lr, None, None, adam_state=st)[0]      # the captured step
    L.inner_step(IDX)
    ll = L.loss_value()
    assert abs(ll - lo) <= 1e-3 * max(1.0, abs(lo)), (ll, lo)
    assert L.adam_t.item() == T0 + 2 and L.plans[8].graph is not None
    L.close()
