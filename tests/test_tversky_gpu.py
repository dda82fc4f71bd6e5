"""The Tversky region term on the device (libmliis_region.so: csrc/tversky.hip, include/mliis_region.h), both entry points against the float64
reference of tests/tversky_ref.py at the shapes of tests/head_instances.py: mliis_tversky_ce through an index vector, over three fold rounds,
33 and 256 partial blocks, saturated logits, without a gradient and with extra_loss; mliis_head_tversky_fused (the sums, their fold, the
gradient tiles) at its predicate's limit, on a partial tile, down- and up-sampling at once, with an empty and a full mask, and refused just
past the limit; every (alpha, beta) of tversky_ref.PAIRS under both.  Then the Learner: one step of Learner(tversky=(0.3, 0.7)) against the
oracle's step composed with the reference loss (fused, fuse_head=False, DARC1, with the focal arguments, Adam), eager against captured and
replayed, the inactive learner, two concurrent lanes against the sequential meta-step, and run_metasegnet.py with the flag.

Bars (those of test_head_instances_gpu.py / test_focal_gpu.py for the same quantities): loss scalars |got - ref| <= 2e-5 * max(1, |ref|);
dlogits / dsmall 1e-4 of the reference's largest entry; the fused head against resize_bilinear_fwd -> tversky_ce -> resize_bilinear_bwd
3e-6; the Learner's step as test_one_focal_step_grads_params_bn.  Every output starts full of NaN or a sentinel, out[3:] and the slack behind
a workspace must keep their sentinel, a second call into differently filled buffers must give the same bits.

Worst figures seen on an MI355X over all cases, for information (bar in brackets; `tversky-figure | ...` lines of a run with -s):
  (not recorded yet)
"""
import contextlib
import functools
import io
import json
import os

import numpy as np
import pytest
import torch

import focal_ref as FR
import tversky_ref as TR

pytestmark = pytest.mark.gpu

from oracle import efficientlab_ref as R  # noqa: E402
from test_head_instances_gpu import FILLS, NAN, SLACK, out_of, same_bits, untouched, workspace  # noqa: E402
from test_ops_gpu import close, dev, f32  # noqa: E402

EXTRA = TR.EXTRA
AB = (0.3, 0.7)      # the learner-level pair
G, W = 2.0, 4.0      # the focal arguments it is combined with


def check(got, ref, tol, what):
    """test_ops_gpu.close with the figure printed beside its bar (shown for a failing test, or with -s)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-30) if g.shape == r.shape else NAN
    print("tversky-figure | {} | {:.3e} | {:.1e}".format(what, err, tol))
    close(got, ref, tol, what)


def check_scalar(got, ref, what):
    """A loss scalar: |got - ref| <= 2e-5 * max(1, |ref|)."""
    got, ref = float(got), float(ref)
    err = abs(got - ref) / max(1.0, abs(ref))
    print("tversky-figure | {} | {:.3e} | {:.1e}".format(what, err, 2e-5))
    assert err <= 2e-5, "{}: {} against {} (err {:.3e} > 2e-5)".format(what, got, ref, err)


# ---------------------------------------------------------------------------------------------------------------- stream-pool bookkeeping
# Every Learner takes a stream from torch's pool of 32, and modules that run behind this one depend on which pool streams they draw
# (tests/test_focal_gpu.py, tests/test_clip_gpu.py).  This module counts the learners it builds -- the ones run_metasegnet builds too -- and
# its last test takes the streams that complete a full turn, so the modules behind it find the pool where a suite without this file leaves it.
_BUILT = [0]


@pytest.fixture(scope="module", autouse=True)
def _count_learners():
    from mliis_amd.learner import Learner
    init = Learner.__init__

    @functools.wraps(init)
    def counted(self, *a, **kw):
        _BUILT[0] += 1
        return init(self, *a, **kw)

    Learner.__init__ = counted
    yield
    Learner.__init__ = init


def _device_case(o, d, key):
    zg, lg = f32(o[key], d), f32(o["labels"], d)
    ig = torch.tensor(o["idx"], dtype=torch.int32, device=d) if o["idx"] else None
    return zg, lg, ig


# ---------------------------------------------------------------------------------------------------------------- mliis_tversky_ce
@pytest.mark.parametrize("c", TR.cases_of("tversky_ce"), ids=TR.case_id)
def test_tversky_ce(c):
    from mliis_amd import ops
    from mliis_amd._lib import region_lib
    d = dev()
    p = c.p
    N, H, W_ = p["N"], p["H"], p["W"]
    o = TR.ce_oracle(c.name)
    zg, lg, ig = _device_case(o, d, "z")
    need = region_lib.size("mliis_tversky_ce_workspace_floats", N, H, W_)

    def run(fills):
        dl, out = out_of(zg.shape, fills[0], d), out_of((4,), fills[1], d)
        ws = workspace(ops, d, need, fills[1])
        got = ops.tversky_ce(zg, lg, ig, p["ls"], p["gamma"], p["fgw"], p["alpha"], p["beta"], p["extra"], want_grad=bool(p["grad"]), dlogits=dl,
                             out=out, ws=ws)
        assert got[0] is out and got[1] is dl and ws.buf.numel() == need + SLACK
        untouched(ws.buf[need:], fills[1], "tversky_ce workspace")
        untouched(out[3:], fills[1], "tversky_ce out[3]")
        if not p["grad"]:
            untouched(dl, fills[0], "tversky_ce dlogits (not asked for)")
        return out[:3].clone(), dl

    first = run(FILLS[0])
    out, dl = first
    assert torch.isfinite(out).all().item()
    check_scalar(out[0], o["loss"], "tversky_ce loss " + c.name)
    check_scalar(out[1], o["pix"], "tversky_ce pixel term " + c.name)
    check_scalar(out[2], o["iou"], "tversky_ce iou " + c.name)
    if p["grad"]:
        assert torch.isfinite(dl).all().item()
        check(dl, o["gz"], 1e-4, "tversky_ce dlogits " + c.name)
        assert torch.equal(dl[..., 0], -dl[..., 1])
    second = run(FILLS[1])
    same_bits([first[0]] + ([dl] if p["grad"] else []), [second[0]] + ([second[1]] if p["grad"] else []), "tversky_ce")


# ---------------------------------------------------------------------------------------------------------------- mliis_head_tversky_fused
@pytest.mark.parametrize("c", TR.cases_of("head"), ids=TR.case_id)
def test_head_tversky_fused(c):
    from mliis_amd import ops
    from mliis_amd._lib import region_lib
    d = dev()
    p = c.p
    N, Hd, Wd, H, W_, ls, gamma, fgw, alpha, beta = (p[k] for k in ("N", "Hd", "Wd", "H", "W", "ls", "gamma", "fgw", "alpha", "beta"))
    o = TR.head_oracle(c.name)
    sg, lg, ig = _device_case(o, d, "small")
    need = region_lib.size("mliis_head_tversky_fused_workspace_floats", N, Hd, Wd, H, W_)
    assert bool(region_lib.size("mliis_head_tversky_fused_supported", Hd, Wd, H, W_)) == (c.inst != "refused")
    if c.inst == "refused":
        ds, out, ws = out_of(sg.shape, NAN, d), out_of((4,), 7.0, d), workspace(ops, d, need, 7.0)
        with pytest.raises(ops.MliisError, match="up-sampling factor too large"):
            ops.head_tversky_fused(sg, lg, ig, (H, W_), ls, gamma, fgw, alpha, beta, ds, out, extra_loss=EXTRA, ws=ws)
        untouched(ds, NAN, "refused head dsmall")
        untouched(out, 7.0, "refused head out")
        untouched(ws.buf, 7.0, "refused head workspace")
        return

    def run(fills):
        ds, out = out_of(sg.shape, fills[0], d), out_of((4,), fills[1], d)
        ws = workspace(ops, d, need, fills[1])
        got = ops.head_tversky_fused(sg, lg, ig, (H, W_), ls, gamma, fgw, alpha, beta, ds, out, extra_loss=EXTRA, ws=ws)
        assert got[0] is out and got[1] is ds and ws.buf.numel() == need + SLACK
        untouched(ws.buf[need:], fills[1], "head workspace")
        untouched(out[3:], fills[1], "head out[3]")
        return ds, out[:3].clone()

    first = run(FILLS[0])
    ds, out = first
    assert all(torch.isfinite(t).all().item() for t in first)
    check(ds, o["gs"], 1e-4, "head dsmall " + c.name)
    check_scalar(out[0], o["loss"], "head loss " + c.name)
    check_scalar(out[1], o["pix"], "head pixel term " + c.name)
    check_scalar(out[2], o["iou"], "head iou " + c.name)
    # the chain the three launches replace
    lo = ops.resize_bilinear_fwd(sg, (H, W_))
    outc = out_of((4,), 7.0, d)
    _, dlc = ops.tversky_ce(lo, lg, ig, ls, gamma, fgw, alpha, beta, EXTRA, want_grad=True, out=outc)
    dsc = ops.resize_bilinear_bwd(dlc, (Hd, Wd))
    check(ds, dsc, 3e-6, "head dsmall vs resize -> tversky_ce -> resize^T " + c.name)
    print("tversky-figure | head vs the chain {}: dsmall bits {} | out bits {}".format(
        c.name, "equal" if torch.equal(ds, dsc) else "differ", "equal" if torch.equal(out, outc[:3]) else "differ"))
    for k, what in enumerate(("loss", "pixel term", "iou")):
        check_scalar(out[k], outc[k], "head {} vs the chain {}".format(what, c.name))
    same_bits(first, run(FILLS[1]), "fused tversky head")


# ---------------------------------------------------------------------------------------------------------------- alpha = beta = 1
@pytest.mark.parametrize("name", ["limit", "n9", "hd2", "mixed-39", "identity"])
def test_at_1_1_on_the_cross_entropy_is_the_dice_chain(name):
    """(1, 1), gamma = 0, W = 1 against the launches --loss_name bce_dice takes today: resize_bilinear_fwd -> softmax_ce(dice) -> resize^T."""
    from mliis_amd import ops
    d = dev()
    p = FR.case(name).p
    sg, lg, ig = _device_case(FR.head_oracle(name), d, "small")
    size = (p["H"], p["W"])
    lo = ops.resize_bilinear_fwd(sg, size)
    want_out, want_dl, _ = ops.softmax_ce(lo, lg, ig, p["ls"], True, EXTRA, want_grad=True)
    want_ds = ops.resize_bilinear_bwd(want_dl, (p["Hd"], p["Wd"]))
    out, ds = ops.head_tversky_fused(sg, lg, ig, size, p["ls"], 0.0, 1.0, 1.0, 1.0, torch.empty_like(sg), out_of((4,), 7.0, d), extra_loss=EXTRA)
    outc, dlc = ops.tversky_ce(lo, lg, ig, p["ls"], 0.0, 1.0, 1.0, 1.0, EXTRA, want_grad=True)
    for k, what in enumerate(("loss", "ce", "iou")):
        check_scalar(out[k], want_out[k], "head_tversky_fused(1, 1) {} vs the dice chain {}".format(what, name))
        check_scalar(outc[k], want_out[k], "tversky_ce(1, 1) {} vs softmax_ce(dice) {}".format(what, name))
    check(ds, want_ds, 1e-4, "head_tversky_fused(1, 1) dsmall vs the dice chain " + name)
    check(dlc, want_dl, 1e-4, "tversky_ce(1, 1) dlogits vs softmax_ce(dice) " + name)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_raise_with_the_outputs_untouched():
    from mliis_amd import ops
    from mliis_amd._lib import region_lib
    d = dev()
    N, H, W_, Hd, Wd = 2, 9, 7, 4, 3
    z, small = torch.zeros(N, H, W_, 2, device=d), torch.zeros(N, Hd, Wd, 2, device=d)
    labels = torch.zeros(N, H, W_, 2, device=d)
    dl, ds, out = out_of(z.shape, NAN, d), out_of(small.shape, NAN, d), out_of((4,), 7.0, d)
    need = region_lib.size("mliis_tversky_ce_workspace_floats", N, H, W_)
    assert need == region_lib.size("mliis_head_tversky_fused_workspace_floats", N, Hd, Wd, H, W_)
    ws = torch.full((need + SLACK,), 5.0, device=d)
    s = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")
    good = dict(N=N, ls=0.0, gamma=G, fgw=W, alpha=AB[0], beta=AB[1], ws=ws.numel(), z=z.data_ptr(), lab=labels.data_ptr(), out=out.data_ptr(),
                wsp=ws.data_ptr(), small=small.data_ptr(), ds=ds.data_ptr(), H=H, W=W_)
    bad = [dict(alpha=-0.5), dict(alpha=nan), dict(alpha=inf), dict(beta=-1.0), dict(beta=nan), dict(beta=inf), dict(alpha=0.0, beta=0.0),
           dict(gamma=-0.5), dict(gamma=nan), dict(gamma=inf), dict(fgw=0.0), dict(fgw=-1.0), dict(fgw=nan), dict(fgw=inf), dict(ls=1.0),
           dict(ls=-0.01), dict(ls=nan), dict(N=0), dict(N=-2), dict(H=0), dict(W=-1), dict(z=None, small=None), dict(lab=None), dict(out=None),
           dict(wsp=None), dict(ws=need - 1), dict(ws=0), dict(wsp=ws.data_ptr() + 4), dict(z=z.data_ptr() + 4, small=small.data_ptr() + 4)]
    for kw in bad:
        a = dict(good)
        a.update(kw)
        with pytest.raises(ops.MliisError, match="mliis_tversky_ce failed"):
            region_lib.call("mliis_tversky_ce", a["z"], a["lab"], None, a["N"], a["H"], a["W"], a["ls"], a["gamma"], a["fgw"], a["alpha"], a["beta"],
                            0.0, dl.data_ptr(), a["out"], a["wsp"], a["ws"], s)
        with pytest.raises(ops.MliisError, match="mliis_head_tversky_fused failed"):
            region_lib.call("mliis_head_tversky_fused", a["small"], a["lab"], None, a["N"], Hd, Wd, a["H"], a["W"], a["ls"], a["gamma"], a["fgw"],
                            a["alpha"], a["beta"], 0.0, a["ds"], a["out"], a["wsp"], a["ws"], s)
    for hd, wd in ((0, Wd), (Hd, -1), (1, Wd)):
        with pytest.raises(ops.MliisError, match="mliis_head_tversky_fused failed"):
            region_lib.call("mliis_head_tversky_fused", good["small"], good["lab"], None, N, hd, wd, H, W_, 0.0, G, W, AB[0], AB[1], 0.0, good["ds"],
                            good["out"], good["wsp"], ws.numel(), s)
    with pytest.raises(ops.MliisError, match="mliis_head_tversky_fused failed"):      # dsmall is required
        region_lib.call("mliis_head_tversky_fused", good["small"], good["lab"], None, N, Hd, Wd, H, W_, 0.0, G, W, AB[0], AB[1], 0.0, None,
                        good["out"], good["wsp"], ws.numel(), s)
    torch.cuda.synchronize()
    untouched(dl, NAN, "refused tversky_ce dlogits")
    untouched(ds, NAN, "refused head dsmall")
    untouched(out, 7.0, "refused out")
    untouched(ws, 5.0, "refused workspace")
    # and the wrappers' own contracts: a strided tensor, a wrong output shape, a wrong dtype
    with pytest.raises(ops.MliisError):
        ops.tversky_ce(z[..., ::1].transpose(1, 2), labels)
    with pytest.raises(ops.MliisError):
        ops.tversky_ce(z, labels, dlogits=torch.empty(N, H, W_ + 1, 2, device=d))
    with pytest.raises(ops.MliisError):
        ops.head_tversky_fused(small, labels, None, (H, W_), 0.0, G, W, AB[0], AB[1], torch.empty(N, Hd, Wd + 1, 2, device=d), out)
    with pytest.raises(ops.MliisError):
        ops.head_tversky_fused(small.double(), labels, None, (H, W_), 0.0, G, W, AB[0], AB[1], ds, out)


# ---------------------------------------------------------------------------------------------------------------- the Learner
def _tversky_oracle_loss(monkeypatch, alpha, beta, gamma=0.0, fgw=1.0):
    """The oracle's loss with the reference region term added and its cross-entropy term replaced by the reference pixel term, for the test's
    duration: every other term (DARC1, L2, L1) stays the oracle's own, composed as it composes them."""
    plain = R.loss_fn
    alpha, beta = FR.as_f32(alpha), FR.as_f32(beta)

    def loss_fn(a, params, logits, labels, label_smoothing=0.0, dice=False, l2=False, l1=False, darc1=False):
        t = labels.to(logits.dtype)
        return (plain(a, params, logits, labels, label_smoothing, False, l2, l1, darc1) - FR.pixel_term(logits, t, label_smoothing, 0.0, 1.0) +
                FR.pixel_term(logits, t, label_smoothing, gamma, fgw) + TR.region_term(logits, t, alpha, beta))

    monkeypatch.setattr(R, "loss_fn", loss_fn)


def _traced_step(L, idx, **kw):
    """One eager step; returns the entry points it called in the step's library, in the loss library and in the region library."""
    from mliis_amd._lib import lib, loss_lib, region_lib
    lib.trace, loss_lib.trace, region_lib.trace = [], [], []
    try:
        L.inner_step(idx, **kw)
        L.synchronize()
        return [n for n, _ in lib.trace], [n for n, _ in loss_lib.trace], [n for n, _ in region_lib.trace]
    finally:
        lib.trace, loss_lib.trace, region_lib.trace = None, None, None


PLAIN_LOSS_CALLS = {"mliis_softmax_ce", "mliis_head_ce_fused", "mliis_final_conv_bwd_data_fin"}


@pytest.mark.parametrize("kw", [dict(), dict(fuse_head=False), dict(darc1=True), dict(focal_gamma=G, fg_weight=W, label_smoothing=0.1)],
                         ids=["fused", "chain", "darc1", "focal"])
def test_one_tversky_step_grads_params_bn(kw, monkeypatch):
    from test_step_gpu import _compare_state, _dc, _pair, _task
    H, S, idx = 64, 5, [3, 1, 4, 0, 2, 3, 1, 1]
    gamma, fgw, ls = kw.get("focal_gamma", 0.0), kw.get("fg_weight", 1.0), kw.get("label_smoothing", 0.0)
    _tversky_oracle_loss(monkeypatch, AB[0], AB[1], gamma, fgw)
    O, L = _pair(H, tversky=AB, **kw)
    assert L.tversky == AB and not L.dice
    x, y = _task(S, H, 1)
    L.load_task(x, y)
    dc = _dc(O, len(idx), 5)
    xb, yb = torch.tensor(x[idx]).double(), torch.tensor(y[idx]).double()
    lo, gO, logits = R.inner_step(O.a, O.params, O.bn, xb, yb, 1e-3, dc, None, ls, False, False, darc1=kw.get("darc1", False))
    step_calls, loss_calls, region_calls = _traced_step(L, idx, dc_scales=dc)
    fused = not (kw.get("fuse_head") is False or kw.get("darc1"))
    assert region_calls == (["mliis_head_tversky_fused"] if fused else ["mliis_tversky_ce"])
    assert loss_calls == [] and not PLAIN_LOSS_CALLS & set(step_calls)
    assert ("mliis_darc1" in step_calls) == bool(kw.get("darc1"))
    ll = L.loss_value()
    print("tversky-figure | step loss {} | {:.3e} | {:.1e}".format(kw, abs(ll - lo) / max(1.0, abs(lo)), 1e-4))
    assert abs(ll - lo) <= 1e-4 * max(1.0, abs(lo)), (ll, lo)
    # out[1], the slot the step log records as `ce`: the pixel term; out[2], its `iou`: the soft IoU, not the Tversky index
    pix = FR.pixel_term(logits.detach(), yb, FR.as_f32(ls), gamma, fgw).item()
    check_scalar(L.last_loss[1].item(), pix, "step pixel term {}".format(kw))
    check_scalar(L.last_loss[2].item(), FR.soft_iou(logits.detach(), yb).item(), "step iou {}".format(kw))
    _compare_state(O, L, gO, "tversky step")
    L.close()


def test_one_tversky_adam_step(monkeypatch):
    from mliis_amd.learner import Learner
    from test_step_gpu import _compare_grads, _task
    H, S, idx = 64, 5, [3, 1, 4, 0, 2, 3, 1, 1]
    _tversky_oracle_loss(monkeypatch, AB[0], AB[1])
    O = R.OracleLearner(image_size=H, seed=0, dtype=torch.float64, lr=1e-3)
    L = Learner(image_size=H, seed=3, optimizer="adam", use_graph=False, drop_connect=False, tversky=AB)
    L.load_named({k: v.numpy() for k, v in O.params.items()}, strict=False)
    x, y = _task(S, H, 1)
    L.load_task(x, y)
    xb, yb = torch.tensor(x[idx]).double(), torch.tensor(y[idx]).double()
    lo, gO, _ = R.inner_step(O.a, O.params, O.bn, xb, yb, 1e-3, None, None, adam_state={"t": 0, "v": {}})
    L.inner_step(idx)
    assert abs(L.loss_value() - lo) <= 1e-4 * max(1.0, abs(lo))
    _compare_grads(L, gO, "tversky adam step")
    th = L.arena.export_trainable_packed().cpu().double()
    ref = torch.cat([O.params[p.name].reshape(-1) for p in L.arena.trainable])
    # (test_step_gpu.py: Adam with beta1 = 0 moves every weight by ~lr * sign(g); an element whose gradient is at fp32 rounding level can flip
    # sign against the oracle and differ by up to 2 * lr in this one step)
    diff = (th - ref).abs()
    assert (diff > 2e-4).double().mean().item() < 2e-3, (diff > 2e-4).double().mean().item()
    assert diff.max().item() <= 2 * 1e-3 + 1e-4
    L.close()


def _state_bits(L):
    st = L.export_all()
    return st["theta"].cpu().clone(), st["bn"].cpu().clone()


def _three_steps(L, task):
    L.load_task(*task)
    losses = []
    for idx in ([0, 1, 2, 3], [4, 0, 1, 2], [3, 4, 0, 1]):
        L.inner_step(idx)
        losses.append(np.float32(L.loss_value()))
    out = _state_bits(L) + (torch.tensor(np.array(losses)), L.last_loss[:3].cpu().clone())
    L.close()
    return out


def test_eager_steps_equal_captured_and_replayed_steps():
    from mliis_amd.learner import Learner
    from test_step_gpu import _task
    task = _task(5, 64, 2)
    kw = dict(image_size=64, seed=7, drop_connect=False, tversky=AB, label_smoothing=0.1)
    eager, graph = _three_steps(Learner(use_graph=False, **kw), task), _three_steps(Learner(use_graph=True, **kw), task)
    for a, b, what in zip(eager, graph, ("theta", "bn", "losses", "out")):
        assert torch.equal(a, b), "three eager steps against eager + captured + replayed: {} differ".format(what)
    assert torch.isfinite(eager[2]).all().item()


def test_inactive_learner_loads_nothing_and_keeps_its_launches():
    """Without the argument: the library is not loaded and the step calls what it called before it existed -- the fused cross-entropy head with
    the fold riding in the final conv's backward-data launch, and with dice=True (--loss_name bce_dice alone) the five-launch chain."""
    from mliis_amd._lib import region_lib
    from mliis_amd.learner import Learner
    from test_step_gpu import _task
    task = _task(5, 64, 2)
    saved = region_lib._dll
    region_lib._dll = None                                # as in a process that never touched the library
    try:
        kw = dict(image_size=64, seed=7, drop_connect=False, use_graph=False)
        A, B, D = Learner(**kw), Learner(tversky=None, **kw), Learner(dice=True, **kw)
        assert A.tversky is None and B.tversky is None and D.tversky is None
        A.load_task(*task)
        step_calls, loss_calls, region_calls = _traced_step(A, [0, 1, 2, 3])
        assert loss_calls == [] and region_calls == []
        assert step_calls.count("mliis_head_ce_fused") == 1 and step_calls.count("mliis_final_conv_bwd_data_fin") == 1
        assert "mliis_softmax_ce" not in step_calls
        D.load_task(*task)
        dice_calls, loss_calls, region_calls = _traced_step(D, [0, 1, 2, 3])
        assert loss_calls == [] and region_calls == []
        # (the decoder resizes feature maps too: the chain adds one transpose to the step's)
        assert dice_calls.count("mliis_softmax_ce") == 1
        assert dice_calls.count("mliis_resize_bilinear_bwd") == step_calls.count("mliis_resize_bilinear_bwd") + 1
        assert not {"mliis_head_ce_fused", "mliis_final_conv_bwd_data_fin"} & set(dice_calls)
        B.load_task(*task)
        B.inner_step([0, 1, 2, 3])
        for idx in ([4, 0, 1, 2], [3, 4, 0, 1]):
            A.inner_step(idx)
            B.inner_step(idx)
        for a, b in zip(_state_bits(A) + (A.last_loss[:3].cpu(),), _state_bits(B) + (B.last_loss[:3].cpu(),)):
            assert torch.equal(a, b)
        assert region_lib._dll is None                    # never loaded
        for ln in (A, B, D):
            ln.close()
    finally:
        if region_lib._dll is None:
            region_lib._dll = saved


def test_concurrent_lanes_equal_the_sequential_meta_step_under_the_tversky_loss():
    """tests/test_step_gpu.py's lanes case at its small size (Gecko, 64 x 64, batch 4), the learner and its lane built with the argument: 3 tasks
    adapted on 2 learners at once give the sequential loop's meta-update bit for bit."""
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask
    from mliis_amd.reptile import Gecko
    from test_step_gpu import _task
    d = torch.device("cuda", 0)
    tasks = []
    for i in range(4):
        x, y = _task(10, 64, 20 + i)
        tasks.append(DeviceTask("t%d" % i, torch.tensor(x).to(d), torch.tensor(y).to(d)))

    def run(n_lanes):
        kw = dict(image_size=64, use_graph=True, drop_connect=False, tversky=AB)
        L = Learner(seed=1, **kw)
        lanes = [Learner(seed=50 + k, **kw) for k in range(n_lanes)]
        meta = Gecko(L, rng_mode="per_task", seed=9, lanes=lanes)
        for _ in range(2):
            meta.train_step(tasks, num_shots=5, inner_batch_size=4, inner_iters=3, meta_step_size=0.5, meta_batch_size=3)
        out = _state_bits(L)
        for ln in [L] + lanes:
            ln.close()
        return out

    a, b = run(0), run(1)
    assert torch.isfinite(a[0]).all().item()
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert torch.equal(a[1], b[1]), float((a[1] - b[1]).abs().max())


def test_main_with_the_tversky_flag(tmp_path):
    import run_metasegnet
    from test_e2e_gpu import BASE
    ckpt = str(tmp_path / "tversky")
    with contextlib.redirect_stdout(io.StringIO()):
        run_metasegnet.main(BASE + ["--sgd", "--meta-iters", "2", "--eval-interval", "0", "--tversky", "0.3", "0.7", "--inner-loop-log",
                                    "--checkpoint", ckpt])
    rows = [json.loads(ln) for ln in open(os.path.join(ckpt, "train", "inner_loop.jsonl"))]
    assert len(rows) == 2
    for row in rows:
        assert np.isfinite(row["loss_last"]) and np.isfinite(row["loss_first"]) and row["nonfinite_steps"] == 0, row


def test_the_stream_pool_is_left_on_a_full_turn():
    """(the last test of the module: see _count_learners)"""
    assert _BUILT[0] > 0
    pad = [torch.cuda.Stream() for _ in range(-_BUILT[0] % 32)]
    print("tversky-figure | learners built by this module {} | streams taken to complete the turn {}".format(_BUILT[0], len(pad)))
    assert (_BUILT[0] + len(pad)) % 32 == 0
