"""A float64 parity case for every launch path of the decoder tail (tests/head_instances.py: the 13 kernels of csrc/head.hip behind
resize forward / backward, the final 1x1 conv, softmax cross-entropy with the dice term, the fused head, DARC1 and the ASPP swish-mask),
at the shapes where the launchers change route and the kernels have their edges: misaligned channel slices, Hi = 1, grid-stride loops that
iterate twice, a 64 KiB LDS launch and the fall-back one column later, candidate rows walked in several rounds, more than 8 and more than
16 images in the loss fold, 33 and 256 partial blocks, every (dice, gradient, mask) launch form, the fused head at the limit of its
predicate and just past it, and DARC1's arg-max with planted winners and exact ties.

References are float64 on seeded, fp32-exact inputs, computed once per case: F.interpolate(align_corners=True) with autograd, a plain
matmul, oracle.efficientlab_ref.loss_fn (out[1] = its cross-entropy term, out[2] = the mean of (I + 1e-7) / (U + 1e-7), also when the
dice term is off), efficientlab_ref.predictions for the mask, the chain interpolate -> loss_fn -> autograd for the fused head, autograd
through efficientlab_ref.swish, and for DARC1 the rule written out: s = |z|.sum(0), position = the FIRST arg-max in flat order, loss term
w * s[pos], gradient w * sign(z[:, pos]) at that one position.  (TensorFlow shares a max gradient among tied positions; the kernel
documents "the first index", and that documented rule is what the tie cases test.)

Bars are the suite's (test_ops_gpu.close, relative to the reference's max-abs): forward 2e-5, gradients 1e-4, loss scalars
2e-5 * max(1, |ref|), swish-mask 2e-6 forward and 1e-5 backward, the fused head against the resize -> softmax_ce -> resize^T chain 3e-6.
Every output starts full of NaN or a sentinel, everything outside a slice and behind a workspace's extent must keep its sentinel, a
second call into differently filled buffers must give the same bits, and the one-launch head (head_ce_fused(finalize=False) ->
final_conv_bwd_data(fin=...)) must give the bits of the two-launch form.

The fused-head case (20,9)->(9,40) is refused by mliis_head_ce_fused_supported (columns up by 39/8, past the predicate's ~4.5), so it is
asserted to raise like (11,11)->(49,49); (20,9)->(9,39), the last admitted column factor, runs the mixed up-/down-sampling path.
A dropout mask beside a channel-slice view goes through the C entry points with the mask in the layout of x (include/mliis_hip.h); the
Python wrappers take dense masks only and refuse that combination.

Worst figures seen on an MI355X over all cases, for information (bar in brackets):
  resize           forward 2.5e-6 (2e-5, the grid-stride case); backward 1.3e-6 overwrite, 7.8e-7 accumulate (1e-4)
  final conv       y 1.3e-7 (2e-5); dx 6.8e-8, dw 9.1e-8, db 3.3e-8 (1e-4)
  softmax CE       loss 4.6e-8, ce 3.4e-8, iou 3.4e-8 (2e-5); dlogits 2.5e-7 (1e-4); mask: no pixel inside the 1e-6 margin but the planted ties
  fused head       dsmall 3.2e-7, dx behind it 3.3e-7 (1e-4); loss 8.6e-8, ce 9.2e-8, iou 1.2e-8 (2e-5); against the chain: the same bits
                   in every case (3e-6); the one-launch form: the same bits
  DARC1            loss term 2.2e-9 (2e-5); dlogits: the same bits as start + weight * sign(z)
  swish-mask       forward 9.7e-8 (2e-6); backward 3.8e-7 (1e-5)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import head_instances as HI

pytestmark = pytest.mark.gpu

from oracle import efficientlab_ref as R  # noqa: E402
from test_dwconv_instances_gpu import FILLS, NAN, SLACK, fp32_exact, out_of, same_bits  # noqa: E402
from test_ops_gpu import close, dev, f32, nchw, nhwc, rnd  # noqa: E402

EXTRA = 0.375


def check(got, ref, tol, what):
    """test_ops_gpu.close with the figure printed beside its bar (shown for a failing test, or with -s)."""
    g, r = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-30) if g.shape == r.shape else NAN
    print("head-figure | {} | {:.3e} | {:.1e}".format(what, err, tol))
    close(got, ref, tol, what)


def check_scalar(got, ref, what):
    """A loss scalar: |got - ref| <= 2e-5 * max(1, |ref|)."""
    got, ref = float(got), float(ref)
    err = abs(got - ref) / max(1.0, abs(ref))
    print("head-figure | {} | {:.3e} | {:.1e}".format(what, err, 2e-5))
    assert err <= 2e-5, "{}: {} against {} (err {:.3e} > 2e-5)".format(what, got, ref, err)


def untouched(t, fill, what):
    ok = torch.isnan(t).all().item() if fill != fill else (t == fill).all().item()
    assert ok, what + ": written where nothing may be written"


def sliced(t, lo, ld, fill, d, pad=NAN):
    """t [..., C] as the view [..., lo:lo + C] of a device tensor of leading dimension ld whose other channels hold `pad`; a None t gives
    a view full of `fill`.  Returns (wide tensor, view)."""
    shape, C = (tuple(t.shape[:-1]), t.shape[-1]) if torch.is_tensor(t) else (tuple(t[:-1]), t[-1])
    wide = torch.full(shape + (ld,), pad, device=d)
    view = wide[..., lo:lo + C]
    if torch.is_tensor(t):
        view.copy_(f32(t, d))
    else:
        view.fill_(fill)
    return wide, view


def outside_untouched(wide, lo, C, sentinel, what):
    assert (wide[..., :lo] == sentinel).all().item() and (wide[..., lo + C:] == sentinel).all().item(), what + ": channels outside the slice were written"


def workspace(ops, d, floats, sentinel):
    ws = ops.Workspace(d, floats=floats + SLACK)
    ws.buf.fill_(sentinel)
    return ws


# ---------------------------------------------------------------------------------------------------------------- resize
@functools.lru_cache(maxsize=None)
def _resize_oracle(N, Hi, Wi, Ho, Wo, C):
    x = fp32_exact(rnd(N, Hi, Wi, C, seed=33)).requires_grad_(True)
    y = F.interpolate(nchw(x), size=(Ho, Wo), mode="bilinear", align_corners=True)
    dy = fp32_exact(rnd(*y.shape, seed=34))
    (gx,) = torch.autograd.grad(y, [x], dy)
    return dict(x=x.detach(), y=nhwc(y.detach()), dy=nhwc(dy), gx=gx.detach(), prev=fp32_exact(rnd(N, Hi, Wi, C, seed=37)))


def _resize_args(c):
    p = c.p
    return p["N"], p["Hi"], p["Wi"], p["Ho"], p["Wo"], p["C"]


@pytest.mark.parametrize("c", HI.cases_of("resize_fwd"), ids=HI.case_id)
def test_resize_forward(c):
    from mliis_amd import ops
    d = dev()
    N, Hi, Wi, Ho, Wo, C = _resize_args(c)
    o = _resize_oracle(N, Hi, Wi, Ho, Wo, C)
    lo, _, ld = HI.SLICE if c.p["sliced"] else (0, C, C)

    def run(fills):
        _, xv = sliced(o["x"], lo, ld, None, d)
        wide, yv = sliced((N, Ho, Wo, C), lo, ld, fills[0], d, pad=fills[1])
        assert HI.route_resize_fwd(C, ld, ld, xv.data_ptr() % 16 == 0 and yv.data_ptr() % 16 == 0) == c.inst
        if c.p["sliced"]:
            assert xv.data_ptr() % 16 == 8 and yv.data_ptr() % 16 == 8
        assert ops.resize_bilinear_fwd(xv, (Ho, Wo), out=yv) is yv
        outside_untouched(wide, lo, C, fills[1], "resize fwd")
        return (yv.clone(),)

    first = run(FILLS[0])
    assert torch.isfinite(first[0]).all().item()
    check(first[0], o["y"], 2e-5, "resize fwd " + c.name)
    same_bits(first, run(FILLS[1]), "resize forward")


@pytest.mark.parametrize("c", HI.cases_of("resize_bwd"), ids=HI.case_id)
def test_resize_backward(c):
    from mliis_amd import ops
    d = dev()
    N, Hi, Wi, Ho, Wo, C = _resize_args(c)
    o = _resize_oracle(N, Hi, Wi, Ho, Wo, C)
    (lo, _, ld), ldy, lody = (HI.SLICE, HI.SLICE[2], HI.SLICE[0]) if c.p["sliced"] else ((HI.BWD_PAD, 0, C + 2 * HI.BWD_PAD), C, 0)

    def run(fills):
        _, dyv = sliced(o["dy"], lody, ldy, None, d)
        wide, dxv = sliced((N, Hi, Wi, C), lo, ld, fills[0], d, pad=fills[1])
        aligned = dyv.data_ptr() % 16 == 0 and dxv.data_ptr() % 16 == 0
        assert HI.route_resize_bwd(N, Hi, Wi, Ho, Wo, C, ldy, ld, aligned) == c.inst and aligned != c.p["sliced"]
        assert ops.resize_bilinear_bwd(dyv, (Hi, Wi), out=dxv) is dxv
        outside_untouched(wide, lo, C, fills[1], "resize bwd, overwrite")
        over = dxv.clone()
        dxv.copy_(f32(o["prev"], d))
        ops.resize_bilinear_bwd(dyv, (Hi, Wi), out=dxv, accumulate=True)
        outside_untouched(wide, lo, C, fills[1], "resize bwd, accumulate")
        return over, dxv.clone()

    first = run(FILLS[0])
    assert all(torch.isfinite(t).all().item() for t in first)
    check(first[0], o["gx"], 1e-4, "resize bwd, overwrite " + c.name)
    check(first[1], o["gx"] + o["prev"], 1e-4, "resize bwd, accumulate " + c.name)
    same_bits(first, run(FILLS[1]), "resize backward")


# ---------------------------------------------------------------------------------------------------------------- final conv
@functools.lru_cache(maxsize=None)
def _final_oracle(rows, C, use_mask):
    x = fp32_exact(rnd(rows, C, seed=35)).requires_grad_(True)
    w = fp32_exact(rnd(1, 1, C, 2, seed=36)).requires_grad_(True)
    b = fp32_exact(rnd(2, seed=37)).requires_grad_(True)
    mask = (torch.rand(rows, C, generator=torch.Generator().manual_seed(38)) > 0.5).double() * 2.0 if use_mask else None
    y = (x * mask if use_mask else x) @ w[0, 0] + b
    dy = fp32_exact(rnd(*y.shape, seed=39))
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], dy)
    return dict(x=x.detach(), w=w.detach(), b=b.detach(), mask=mask, y=y.detach(), dy=dy, gx=gx, gw=gw, gb=gb)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("c", HI.cases_of("final_conv"), ids=HI.case_id)
def test_final_conv(c):
    from mliis_amd import ops
    d = dev()
    rows, C, ld, lo = c.p["rows"], c.p["C"], c.p["ld"], c.p["off"]
    o = _final_oracle(rows, C, c.p["mask"])
    wg, bg, dyg = f32(o["w"], d), f32(o["b"], d), f32(o["dy"], d)
    strided_mask = c.p["mask"] and ld != C      # the C entry points, the mask in the layout of x: the wrappers take dense masks only

    def run(fills):
        _, xv = sliced(o["x"], lo, ld, None, d)
        mv = sliced(o["mask"], lo, ld, None, d)[1] if c.p["mask"] else None
        y = out_of((rows, 2), fills[0], d)
        wide, dxv = sliced((rows, C), lo, ld, fills[0], d, pad=fills[1])
        dw, db = out_of((1, 1, C, 2), fills[0], d), out_of((2,), fills[0], d)
        if strided_mask:
            ops.lib.call("mliis_final_conv_fwd", xv.data_ptr(), ld, mv.data_ptr(), wg.data_ptr(), bg.data_ptr(), y.data_ptr(), rows, C, _stream())
            ops.lib.call("mliis_final_conv_bwd_data", dyg.data_ptr(), wg.data_ptr(), mv.data_ptr(), dxv.data_ptr(), ld, rows, C, _stream())
            ws = workspace(ops, d, ops.lib.size("mliis_colreduce_workspace_floats", rows, C, 1, 2), fills[1])
            ops.lib.call("mliis_final_conv_bwd_filter", xv.data_ptr(), ld, mv.data_ptr(), dyg.data_ptr(), rows, C, dw.data_ptr(), db.data_ptr(),
                         ws.buf.data_ptr(), ws.buf.numel() - SLACK, _stream())
            assert (ws.buf[-SLACK:] == fills[1]).all().item(), "filter gradient: written past the workspace"
            dense = f32(o["mask"], d)
            for call in (lambda: ops.final_conv_fwd(xv, wg, bg, dense), lambda: ops.final_conv_bwd_data(dyg, wg, C, dense, out=dxv),
                         lambda: ops.final_conv_bwd_filter(xv, dyg, dense)):
                with pytest.raises(ops.MliisError, match="dense activation"):
                    call()
        else:
            assert ops.final_conv_fwd(xv, wg, bg, mv, out=y) is y
            assert ops.final_conv_bwd_data(dyg, wg, C, mv, out=dxv) is dxv
            ops.final_conv_bwd_filter(xv, dyg, mv, dw=dw, db=db)
        outside_untouched(wide, lo, C, fills[1], "final conv dx")
        return y, dxv.clone(), dw, db

    first = run(FILLS[0])
    assert all(torch.isfinite(t).all().item() for t in first)
    check(first[0], o["y"], 2e-5, "final conv fwd " + c.name)
    check(first[1], o["gx"], 1e-4, "final conv dx " + c.name)
    check(first[2], o["gw"], 1e-4, "final conv dw " + c.name)
    check(first[3], o["gb"], 1e-4, "final conv db " + c.name)
    same_bits(first, run(FILLS[1]), "final conv")


# ---------------------------------------------------------------------------------------------------------------- softmax cross-entropy
def _labels(S, H, W, seed, soft):
    m = torch.rand(S, H, W, generator=torch.Generator().manual_seed(seed)).double()
    m = torch.where(m < 0.6, (m < 0.3).double(), m) if soft else (m > 0.6).double()      # mostly binary, some fractional labels
    return fp32_exact(torch.stack([1 - m, m], -1))


def _index(N, S, use):
    return [(3 * i + 1) % S for i in range(N)] if use else None


def _loss_terms(logits, labels, ls, dice):
    """(loss, ce, iou) of efficientlab_ref.loss_fn; ce and iou written out from its formulas (iou also when the dice term is off)."""
    loss = R.loss_fn(R.arch(), {}, logits, labels, ls, bool(dice), False)
    t = labels * (1 - ls) + ls / 2 if ls else labels
    ce = -(t * F.log_softmax(logits, dim=-1)).sum(-1).mean()
    p1, t1 = torch.softmax(logits, dim=-1)[..., 1].flatten(1), labels[..., 1].flatten(1)
    inter = (p1 * t1).sum(1)
    iou = ((inter + 1e-7) / (p1.sum(1) + t1.sum(1) - inter + 1e-7)).mean()
    return loss, ce.detach(), iou.detach()


@functools.lru_cache(maxsize=None)
def _ce_oracle(name):
    p = {c.name: c for c in HI.cases_of("softmax_ce")}[name].p
    N, S, H, W = p["N"], p["S"], p["H"], p["W"]
    z = fp32_exact(rnd(N, H, W, 2, seed=40) * p["zscale"])
    tied = torch.zeros(N, H, W, dtype=torch.bool)
    if p["ties"]:
        tied = torch.rand(N, H, W, generator=torch.Generator().manual_seed(42)) < p["ties"]
        z[..., 1] = torch.where(tied, z[..., 0], z[..., 1])
        assert abs(tied.double().mean().item() - p["ties"]) < 0.02 and (z[..., 0] == z[..., 1])[tied].all()
    labels = _labels(S, H, W, 41, True)
    idx = _index(N, S, p["idx"])
    zr = z.clone().requires_grad_(True)
    loss, ce, iou = _loss_terms(zr, labels[idx] if idx else labels, p["ls"], p["dice"])
    (gz,) = torch.autograd.grad(loss, [zr])
    return dict(z=z, labels=labels, idx=idx, loss=loss.item() + p["extra"], ce=ce.item(), iou=iou.item(), gz=gz, pred=R.predictions(z), tied=tied)


def check_mask(pred, z, ref_pred, tied, what):
    """Bit-equal to the oracle's rule wherever |z0 - z1| > 1e-6, (0, 0) where the logits are exactly equal; apart from planted ties
    fewer than 0.1 % of the pixels may fall inside the margin."""
    pred = pred.cpu()
    zf = z.float()
    margin = (zf[..., 0] - zf[..., 1]).abs() > 1e-6
    equal = zf[..., 0] == zf[..., 1]
    assert torch.equal(pred[margin], ref_pred.float()[margin]), what + ": mask differs from the oracle's rule outside the margin"
    assert (pred[equal] == 0).all().item(), what + ": equal logits must give (0, 0)"
    assert torch.equal(equal & tied, tied)
    left_out = (~margin & ~tied).double().mean().item()
    print("head-figure | {} pixels inside the 1e-6 margin | {:.3e} | {:.1e}".format(what, left_out, 1e-3))
    assert left_out < 1e-3
    assert ((pred == 0) | (pred == 1)).all().item()


@pytest.mark.parametrize("c", HI.cases_of("softmax_ce"), ids=HI.case_id)
def test_softmax_ce(c):
    from mliis_amd import ops
    d = dev()
    p = c.p
    N, H, W = p["N"], p["H"], p["W"]
    o = _ce_oracle(c.name)
    zg, lg = f32(o["z"], d), f32(o["labels"], d)
    ig = torch.tensor(o["idx"], dtype=torch.int32, device=d) if o["idx"] else None
    need = HI.softmax_ce_workspace_floats(N, H, W)
    assert HI.softmax_ce_launches(p["dice"], p["grad"], p["pred"]) == c.inst

    def run(fills):
        dl, pr, out = out_of(zg.shape, fills[0], d), out_of(zg.shape, fills[0], d), out_of((4,), fills[1], d)
        ws = workspace(ops, d, need, fills[1])
        ops.softmax_ce(zg, lg, ig, p["ls"], bool(p["dice"]), p["extra"], want_grad=bool(p["grad"]), want_pred=bool(p["pred"]), dlogits=dl, pred=pr,
                       out=out, ws=ws)
        assert ws.buf.numel() == need + SLACK
        untouched(ws.buf[need:], fills[1], "softmax_ce workspace")
        untouched(out[3:], fills[1], "softmax_ce out[3]")
        if not p["grad"]:
            untouched(dl, fills[0], "softmax_ce dlogits (not asked for)")
        if not p["pred"]:
            untouched(pr, fills[0], "softmax_ce pred (not asked for)")
        return out[:3].clone(), dl, pr

    first = run(FILLS[0])
    out, dl, pr = first
    check_scalar(out[0], o["loss"], "softmax_ce loss " + c.name)
    check_scalar(out[1], o["ce"], "softmax_ce ce " + c.name)
    check_scalar(out[2], o["iou"], "softmax_ce iou " + c.name)
    if p["grad"]:
        assert torch.isfinite(dl).all().item()
        check(dl, o["gz"], 1e-4, "softmax_ce dlogits " + c.name)
    if p["pred"]:
        check_mask(pr, o["z"], o["pred"], o["tied"], "softmax_ce mask " + c.name)
    second = run(FILLS[1])
    same_bits([first[0]] + ([dl] if p["grad"] else []) + ([pr] if p["pred"] else []),
              [second[0]] + ([second[1]] if p["grad"] else []) + ([second[2]] if p["pred"] else []), "softmax_ce")


# ---------------------------------------------------------------------------------------------------------------- fused head
@functools.lru_cache(maxsize=None)
def _head_oracle(name):
    p = {c.name: c for c in HI.cases_of("head")}[name].p
    N, S, Hd, Wd, H, W = p["N"], p["S"], p["Hd"], p["Wd"], p["H"], p["W"]
    small = fp32_exact(rnd(N, Hd, Wd, 2, seed=90) * 3)
    labels = _labels(S, H, W, 91, False)
    idx = _index(N, S, p["idx"])
    sm = small.clone().requires_grad_(True)
    logits = nhwc(F.interpolate(nchw(sm), size=(H, W), mode="bilinear", align_corners=True))
    loss, ce, iou = _loss_terms(logits, labels[idx] if idx else labels, p["ls"], False)
    (gs,) = torch.autograd.grad(loss, [sm])
    w = fp32_exact(rnd(1, 1, 8, 2, seed=92))
    return dict(small=small, labels=labels, idx=idx, loss=loss.item() + EXTRA, ce=ce.item(), iou=iou.item(), gs=gs, w=w, gx=gs @ w[0, 0].t())


@pytest.mark.parametrize("c", HI.cases_of("head"), ids=HI.case_id)
def test_head_ce_fused(c):
    from mliis_amd import ops
    d = dev()
    p = c.p
    N, Hd, Wd, H, W, ls = p["N"], p["Hd"], p["Wd"], p["H"], p["W"], p["ls"]
    o = _head_oracle(c.name)
    sg, lg, wg = f32(o["small"], d), f32(o["labels"], d), f32(o["w"], d)
    ig = torch.tensor(o["idx"], dtype=torch.int32, device=d) if o["idx"] else None
    need = HI.head_workspace_floats(N, Hd, Wd)
    assert bool(ops.lib.raw("mliis_head_ce_fused_supported")(Hd, Wd, H, W)) == (c.inst == "head") == HI.head_supported(Hd, Wd, H, W)
    if c.inst == "head-refused":
        ds, out = out_of(sg.shape, NAN, d), out_of((4,), 7.0, d)
        with pytest.raises(ops.MliisError, match="up-sampling factor too large"):
            ops.head_ce_fused(sg, lg, ig, (H, W), ls, ds, out, extra_loss=EXTRA, ws=workspace(ops, d, need, 7.0))
        untouched(ds, NAN, "refused head dsmall")
        untouched(out, 7.0, "refused head out")
        return

    def run(fills):
        # two launches: head_ce_fused_k -> ce_finalize_k
        ds, out = out_of(sg.shape, fills[0], d), out_of((4,), fills[1], d)
        ws = workspace(ops, d, need, fills[1])
        ops.head_ce_fused(sg, lg, ig, (H, W), ls, ds, out, extra_loss=EXTRA, ws=ws)
        dx = ops.final_conv_bwd_data(ds, wg, 8, out=out_of((N, Hd, Wd, 8), fills[0], d))
        # one launch, the fold rides in the final conv's backward-data
        ds1, out1 = out_of(sg.shape, fills[0], d), out_of((4,), fills[1], d)
        ws1 = workspace(ops, d, need, fills[1])
        _, _, buf = ops.head_ce_fused(sg, lg, ig, (H, W), ls, ds1, out1, extra_loss=EXTRA, ws=ws1, finalize=False)
        untouched(out1, fills[1], "one-launch head: out before the fold")
        dx1 = ops.final_conv_bwd_data(ds1, wg, 8, out=out_of((N, Hd, Wd, 8), fills[0], d), fin=(buf, (H, W), EXTRA, out1))
        for w_ in (ws, ws1):
            assert w_.buf.numel() == need + SLACK
            untouched(w_.buf[need:], fills[1], "head workspace")
        untouched(out[3:], fills[1], "head out[3]")
        untouched(out1[3:], fills[1], "one-launch head out[3]")
        assert torch.equal(ds1, ds), "one-launch head: dsmall differs from the two-launch form"
        assert torch.equal(out1[:3], out[:3]), "one-launch head: out differs from the two-launch form: {} {}".format(out1, out)
        assert torch.equal(dx1, dx), "final_conv_bwd_data(fin=...) dx differs from the plain call"
        return ds, out[:3].clone(), dx

    first = run(FILLS[0])
    ds, out, dx = first
    assert all(torch.isfinite(t).all().item() for t in first)
    check(ds, o["gs"], 1e-4, "head dsmall " + c.name)
    check(dx, o["gx"], 1e-4, "head -> final conv dx " + c.name)
    check_scalar(out[0], o["loss"], "head loss " + c.name)
    check_scalar(out[1], o["ce"], "head ce " + c.name)
    check_scalar(out[2], o["iou"], "head iou " + c.name)
    # the chain the fused launch replaces
    lo = ops.resize_bilinear_fwd(sg, (H, W))
    outc = out_of((4,), 7.0, d)
    _, dl, _ = ops.softmax_ce(lo, lg, ig, ls, False, EXTRA, want_grad=True, out=outc)
    check(ds, ops.resize_bilinear_bwd(dl, (Hd, Wd)), 3e-6, "head dsmall vs resize -> softmax_ce -> resize^T " + c.name)
    for k, what in enumerate(("loss", "ce", "iou")):
        check_scalar(out[k], outc[k], "head {} vs the chain {}".format(what, c.name))
    same_bits(first, run(FILLS[1]), "fused head")


# ---------------------------------------------------------------------------------------------------------------- DARC1
@functools.lru_cache(maxsize=None)
def _darc1_oracle(name):
    p = {c.name: c for c in HI.cases_of("darc1")}[name].p
    N, H, W = p["N"], p["H"], p["W"]
    z = fp32_exact(rnd(N, H, W, 2, seed=120))
    col = torch.tensor([6.5 * (1 if n % 2 == 0 else -1) for n in range(N)], dtype=torch.float64)
    if p["zero"]:
        col[2] = 0.0
    flat = z.view(N, -1)
    for q in p["plant"]:
        flat[:, q] = col
    s = flat.abs().sum(0)
    pos = int((s == s.max()).nonzero()[0])
    # the winner is planted, not hoped for: it leads every unplanted position by 1e-3 of its value, and planted positions tie exactly
    # with dyadic terms whose fp32 sum is exact -- an fp32 summation difference cannot move the arg-max
    rest = s.clone()
    rest[list(p["plant"])] = 0.0
    assert pos == p["plant"][0] and (s[list(p["plant"])] == s.max()).all() and s.max().item() == 6.5 * (N - (1 if p["zero"] else 0))
    assert s.max().item() - rest.max().item() >= 1e-3 * s.max().item()
    assert (col[1::2] < 0).all() or N == 1
    start = (rnd(N, H, W, 2, seed=121) * 64).round() / 64
    sign = torch.sign(flat[:, pos])
    wf = float(torch.tensor(p["weight"], dtype=torch.float32))          # the weight as the C ABI's float
    want = start.clone()
    want.view(N, -1)[:, pos] += wf * sign
    return dict(z=z, pos=pos, s=s.max().item(), start=start, want=want, wf=wf)


@pytest.mark.parametrize("c", HI.cases_of("darc1"), ids=HI.case_id)
def test_darc1(c):
    from mliis_amd import ops
    d = dev()
    p = c.p
    o = _darc1_oracle(c.name)
    zg = f32(o["z"], d)
    assert HI.darc1_nblk(zg[0].numel()) == min(HI.cdiv(zg[0].numel(), 256), 1024)
    out0 = (1.25, 7.0, 7.0, 7.0)

    def run(fills):
        dl = f32(o["start"], d) if p["outs"] != "out" else None
        out = torch.tensor(out0, device=d) if p["outs"] != "dlogits" else None
        ws = workspace(ops, d, 2048, fills[1])
        ops.darc1(zg, p["weight"], dlogits=dl, out=out, ws=ws)
        untouched(ws.buf[2048:], fills[1], "darc1 workspace")
        return [t for t in (dl, out) if t is not None]

    first = run(FILLS[0])
    if p["outs"] != "out":
        dl = first[0].cpu()
        changed = (dl != o["start"].float()).view(p["N"], -1).nonzero()
        assert set(changed[:, 1].tolist()) <= {o["pos"]}, "dlogits changed away from the first arg-max {}: at {}".format(o["pos"], sorted(set(changed[:, 1].tolist()))[:8])
        check(dl, o["want"], 1e-4, "darc1 dlogits " + c.name)
        # start + w * sign is one rounding of an exact sum: the same bits
        assert torch.equal(dl, o["want"].float()), "darc1 dlogits: not start + weight * sign(z) at the winner"
        assert len(changed) == p["N"] - (1 if p["zero"] else 0)
    if p["outs"] != "dlogits":
        out = first[-1].cpu()
        check_scalar(out[0], out0[0] + o["wf"] * o["s"], "darc1 loss term " + c.name)
        assert out[1:].tolist() == list(out0[1:]), "darc1 wrote out[1:]"
    same_bits(first, run(FILLS[1]), "darc1")


# ---------------------------------------------------------------------------------------------------------------- swish-mask
@functools.lru_cache(maxsize=None)
def _swish_inputs(rows, C):
    z = fp32_exact(rnd(rows, C, seed=70, scale=2.0))
    mask = (torch.rand(rows, C, generator=torch.Generator().manual_seed(72)) < 0.5).double() * 2.0
    return z, mask, fp32_exact(rnd(rows, C, seed=71))


@functools.lru_cache(maxsize=None)
def _swish_oracle(rows, C, pre, use_mask):
    z, mask, dy = _swish_inputs(rows, C)
    zr = z.clone().requires_grad_(True)
    m = mask if use_mask else torch.ones_like(mask)
    y = R.swish(zr * m) if pre else R.swish(zr) * m
    (gz,) = torch.autograd.grad(y, [zr], dy)
    return y.detach(), gz


@pytest.mark.parametrize("c", HI.cases_of("swish_mask"), ids=HI.case_id)
def test_swish_mask(c):
    from mliis_amd import ops
    d = dev()
    rows, C, ld, lo, pre = c.p["rows"], c.p["C"], c.p["ld"], c.p["off"], bool(c.p["pre"])
    z, mask, dy = _swish_inputs(rows, C)
    y, gz = _swish_oracle(rows, C, c.p["pre"], c.p["mask"])

    def run(fills):
        _, zv = sliced(z, lo, ld, None, d)
        mv = sliced(mask, lo, ld, None, d)[1] if c.p["mask"] else None
        _, dyv = sliced(dy, lo, ld, None, d)
        ywide, yv = sliced((rows, C), lo, ld, fills[0], d, pad=fills[1])
        gwide, gv = sliced((rows, C), lo, ld, fills[0], d, pad=fills[1])
        assert ops.swish_mask_fwd(zv, mv, out=yv, pre_mask=pre) is yv
        assert ops.swish_mask_bwd(dyv, zv, mv, out=gv, pre_mask=pre) is gv
        outside_untouched(ywide, lo, C, fills[1], "swish-mask fwd")
        outside_untouched(gwide, lo, C, fills[1], "swish-mask bwd")
        return yv.clone(), gv.clone()

    first = run(FILLS[0])
    assert all(torch.isfinite(t).all().item() for t in first)
    check(first[0], y, 2e-6, "swish-mask fwd " + c.name)
    check(first[1], gz, 1e-5, "swish-mask bwd " + c.name)
    same_bits(first, run(FILLS[1]), "swish-mask")
