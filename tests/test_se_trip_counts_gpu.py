"""The squeeze-excite MLP kernels request only the weights their C and R fill (se.hip: wave-uniform trip counts).  mliis_se_mlp_fwd,
mliis_se_mlp_bwd (a finished gate gradient, and row-group partials whose groups straddle images: HW = 196 and HW = 16) and
mliis_se_mlp_bwd_bn against float64 at the sizes where the counts change: a single wave, a ragged last wave, the two 14x14 layers of
EfficientLab-6-3, a C that is no multiple of 64 under a full R, and the largest layer of the one-channel-per-thread form.  Every input
ends at a guard band of NaN (a clamped or skipped index that leaves [N, C] / [C, R] reads it), every output is allocated NaN in front of a
guard band that must come back untouched (tests/memcheck.py).  Tolerances: those of test_ops_gpu.test_se (forward 2e-5, backward 1e-4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import memcheck as M  # noqa: E402
from oracle import efficientlab_ref as R  # noqa: E402
from test_ops_gpu import close, dev, rnd  # noqa: E402

CASES = [(1, 16, 4), (2, 40, 10), (8, 480, 20), (8, 672, 28), (3, 1000, 32), (8, 1024, 32)]


def _swish_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _gin(t):
    return M.guarded_input(t.float())


def _backward_ref(dgate, gate, hpre, w1, w2, hw):
    dpre2 = dgate * gate * (1 - gate)
    dpre1 = (dpre2 @ w2.t()) * _swish_grad(hpre)
    return dict(dpre1=dpre1, dpre2=dpre2, chan_add=(dpre1 @ w1.t()) / hw)


@pytest.mark.parametrize("N,C,Rr", CASES)
def test_se_mlp_forward(N, C, Rr):
    from mliis_amd import ops
    dev()
    s, w1, b1 = rnd(N, C, seed=31), rnd(C, Rr, seed=32, scale=0.3), rnd(Rr, seed=33)
    w2, b2 = rnd(Rr, C, seed=34, scale=0.3), rnd(C, seed=35)
    h = s.float().double() @ w1.float().double() + b1.float().double()
    gate = torch.sigmoid(R.swish(h) @ w2.float().double() + b2.float().double())
    M.reset_guards()
    sg, w1g, b1g, w2g, b2g = _gin(s), _gin(w1.view(1, 1, C, Rr)), _gin(b1), _gin(w2.view(1, 1, Rr, C)), _gin(b2)
    snap = M.snapshot(sg, w1g, b1g, w2g, b2g)
    with M.poisoned_allocations():
        hp, gg = ops.se_mlp_fwd(sg, w1g, b1g, w2g, b2g)
        # per-image partial sums [N][chunks][C] folded by the kernel (11 chunks: one full batch of eight and a ragged one)
        chunks = 11
        sp = rnd(N, chunks, C, seed=36)
        s_out = torch.empty(N, C, device="cuda")
        hp2, gg2 = ops.se_mlp_fwd(_gin(sp), w1g, b1g, w2g, b2g, chunks=chunks, scale=0.25, s_out=s_out)
    M.assert_guards()
    snap.assert_unchanged()
    close(hp, h, 2e-5, "se hpre")
    close(gg, gate, 2e-5, "se gate")
    s2 = sp.float().double().sum(1) * 0.25
    h2 = s2 @ w1.float().double() + b1.float().double()
    close(s_out, s2, 2e-5, "se pooled vector from partial sums")
    close(hp2, h2, 2e-5, "se hpre from partial sums")
    close(gg2, torch.sigmoid(R.swish(h2) @ w2.float().double() + b2.float().double()), 2e-5, "se gate from partial sums")


@pytest.mark.parametrize("N,C,Rr", CASES)
def test_se_mlp_backward(N, C, Rr):
    from mliis_amd import ops
    dev()
    f = lambda t: t.float().double()   # noqa: E731  (the float64 reference starts from the float32 values the device sees)
    gate, hpre, s = f(torch.sigmoid(rnd(N, C, seed=41))), f(rnd(N, Rr, seed=42)), f(rnd(N, C, seed=43))
    w1, w2 = f(rnd(C, Rr, seed=44, scale=0.3)), f(rnd(Rr, C, seed=45, scale=0.3))
    M.reset_guards()
    gateg, hpg, sg = _gin(gate), _gin(hpre), _gin(s)
    w1g, w2g, w1tg = _gin(w1.view(1, 1, C, Rr)), _gin(w2.view(1, 1, Rr, C)), _gin(w1.t().contiguous())
    # ---- a finished gate gradient [N, C], with the four weight gradients
    dgate = f(rnd(N, C, seed=46))
    dgg = _gin(dgate)
    snap = M.snapshot(gateg, hpg, sg, w1g, w2g, w1tg, dgg)
    with M.poisoned_allocations():
        o = ops.se_mlp_bwd(dgg, gateg, sg, hpg, w1g, w2g, 49)
        ot = ops.se_mlp_bwd(dgg, gateg, sg, hpg, w1g, w2g, 49, w1t=w1tg)
    M.assert_guards()
    ref = _backward_ref(dgate, gate, hpre, w1, w2, 49)
    ref.update(dw1=(s.t() @ ref["dpre1"]).view(1, 1, C, Rr), db1=ref["dpre1"].sum(0),
               dw2=(R.swish(hpre).t() @ ref["dpre2"]).view(1, 1, Rr, C), db2=ref["dpre2"].sum(0))
    for k in ref:
        close(o[k], ref[k], 1e-4, "se_mlp_bwd " + k)
        assert torch.equal(o[k], ot[k]), "se_mlp_bwd with the transposed w1: " + k
    # ---- row-group partials [groups][2][C]: slot 0 = the rows of the image a 16-row group starts in, slot 1 = its rows of the next image
    for hw in (196, 16):
        rows = f(rnd(N * hw, C, seed=47))
        groups = -(-N * hw // 16)
        part = torch.zeros(groups, 2, C, dtype=torch.float64)
        for rg in range(groups):
            lo, hi = rg * 16, min(rg * 16 + 16, N * hw)
            cut = min(hi, (lo // hw + 1) * hw)
            part[rg, 0] = f(rows[lo:cut].sum(0))
            if cut < hi:
                part[rg, 1] = f(rows[cut:hi].sum(0))
        dgate = torch.zeros(N, C, dtype=torch.float64)
        for rg in range(groups):
            n0 = (rg * 16) // hw
            dgate[n0] += part[rg, 0]
            if n0 + 1 < N:
                dgate[n0 + 1] += part[rg, 1]
        partg = _gin(part)
        snap2 = M.snapshot(partg)
        with M.poisoned_allocations():
            outs = {k: torch.empty(shape, device="cuda") for k, shape in (("dpre1", (N, Rr)), ("dpre2", (N, C)), ("chan_add", (N, C)))}
            ops.se_mlp_bwd(partg, gateg, sg, hpg, w1g, w2g, hw, outs=outs, dgate_groups=groups, w1t=w1tg)
        M.assert_guards()
        snap2.assert_unchanged()
        ref = _backward_ref(dgate, gate, hpre, w1, w2, hw)
        for k in ref:
            close(outs[k], ref[k], 1e-4, "se_mlp_bwd, row-group partials, HW = {}: {}".format(hw, k))
    # ---- the sums of mliis_se_bn_bwd_sums [N][nblk][5][C]: value 0 is the gate gradient, 1..4 give stage 1 of the depthwise batch norm
    for nblk in (1, 7):
        sums = f(rnd(N, nblk, 5, C, seed=48))
        sumsg = _gin(sums)
        with M.poisoned_allocations():
            outs = {k: torch.empty(shape, device="cuda") for k, shape in (("dpre1", (N, Rr)), ("dpre2", (N, C)), ("chan_add", (N, C)))}
            stage1 = torch.empty(N, 2, C, device="cuda")
            ops.se_mlp_bwd_bn(sumsg, nblk, gateg, hpg, w1g, w2g, 196, outs, stage1, w1t=w1tg)
            outs_p, stage1_p = {k: torch.empty_like(v) for k, v in outs.items()}, torch.empty_like(stage1)
            ops.se_mlp_bwd_bn(sumsg, nblk, gateg, hpg, w1g, w2g, 196, outs_p, stage1_p)
        M.assert_guards()
        S = sums.sum(1)
        ref = _backward_ref(S[:, 0], gate, hpre, w1, w2, 196)
        for k in ref:
            close(outs[k], ref[k], 1e-4, "se_mlp_bwd_bn, {} chunks: {}".format(nblk, k))
            assert torch.equal(outs[k], outs_p[k]), "se_mlp_bwd_bn with the transposed w1: " + k
        st_ref = torch.stack([gate * S[:, 1] + ref["chan_add"] * S[:, 3], gate * S[:, 2] + ref["chan_add"] * S[:, 4]], dim=1)
        close(stage1, st_ref, 1e-4, "se_mlp_bwd_bn stage 1, {} chunks".format(nblk))
        assert torch.equal(stage1, stage1_p)
    snap.assert_unchanged()
