"""The row-marching depthwise kernel instances (csrc/dwmarch.hip) as a table, a mirror of the launch geometry that says how many steps
a workgroup marches, and the float64 references of the three entry points.  Shared by test_dwmarch_instances_cpu.py (the table and
the mirror against the library's block queries: host code, no GPU) and test_dwmarch_instances_gpu.py (one parity case per instance
and shape).

Why step counts matter.  dwm_conv_k and dwm_bwd_s2_k run a software pipeline: the prologue issues the loads of steps 0, 1 and 2, and
every loop iteration computes two steps, commits the batch of the next step into the LDS ring and issues the loads of the step three
ahead.  A load issued INSIDE the loop is consumed only by a chunk of at least four steps, and the ring (NR = 10 / 12 rows at stride 1,
17 / 19 at stride 2, 5 / 6 in the stride-2 backward) comes round to a used slot only then.  march_split cuts the rows into chunks of
two steps until 448 (forward) / 256 (backward) workgroups exist, so small test shapes never get there: `geom_fwd` / `geom_bwd` below
make that checkable, and SHAPES holds, per stride, an `edge` shape (bands, chunks, channel tail, two steps) and a `long` shape whose
N * ceil(C / 32) * bands = 240 leaves one chunk per (image, band) that marches 5 to 9 steps.

The mirror only picks shapes: every case also asserts N * bands * chunks against mliis_dwconv_bn_fwd_blocks / _bwd_blocks, so a
change of march_split fails loudly instead of quietly shortening the marches."""
import collections
import itertools
import os

ENV_TARGET = "MLIIS_DWM_TARGET"       # (read once per process by the library: moves the chunk counts away from the mirror's)
TARGET_FWD, TARGET_BWD = 448, 256     # dwm_target()

KS, STRIDES = (3, 5), (1, 2)
# storage types (ta, tb).  Forward: ta = the ring-side input z, tb = the output y.  Backward: ta = dy (fused: da2 and z1), tb = z and dx.
FWD_PAIRS = (("f32", "f32"), ("bf16", "bf16"), ("f32", "bf16"))
BWD_PAIRS = (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"))

# entry: "fwd" = mliis_dwconv_bn_fwd, "bwd" = mliis_dwconv_bn_bwd, "fused" = mliis_mbconv_dw_bwd_march (always with the batch norm)
Instance = collections.namedtuple("Instance", "entry k s bn ta tb")


def types_ok(bwd, ta, tb):
    """dwm_types_ok: both fp32, both bf16, or the one mixed pair of the direction (forward fp32 -> bf16, backward bf16 dy with fp32 z / dx)."""
    if ta == tb:
        return True
    return (ta, tb) == (("bf16", "f32") if bwd else ("f32", "bf16"))


def kernel_name(i):
    """The template instance an Instance launches (launch_conv / launch_bwd_s2 / launch_bwd_dybn_t)."""
    t = {"f32": "float", "bf16": "bf16s"}
    b = {True: "true", False: "false"}
    if i.entry == "fwd":
        return "dwm_conv_k<{}, {}, {}, false, false, {}, {}>".format(i.k, i.s, b[i.bn], t[i.ta], t[i.tb])
    dybn = i.entry == "fused"
    if i.s == 1:
        return "dwm_conv_k<{}, 1, {}, true, {}, {}, {}>".format(i.k, b[i.bn], b[dybn], t[i.ta], t[i.tb])
    return "dwm_bwd_s2_k<{}, {}, {}, {}, {}>".format(i.k, b[i.bn], b[dybn], t[i.ta], t[i.tb])


def declared():
    """Everything the launch switches at the end of dwmarch.hip can name: 24 + 12 + 12 + 12 = 60 instances."""
    out = [Instance("fwd", k, s, bn, ta, tb) for k, s, bn, (ta, tb) in itertools.product(KS, STRIDES, (True, False), FWD_PAIRS)]
    out += [Instance("bwd", k, s, bn, ta, tb) for s, k, bn, (ta, tb) in itertools.product(STRIDES, KS, (True, False), BWD_PAIRS)]
    out += [Instance("fused", k, s, True, ta, tb) for k, s, (ta, tb) in itertools.product(KS, STRIDES, BWD_PAIRS)]
    return tuple(out)


INSTANCES = declared()
# instance -> why no operator-level call can launch it.  Empty: the storage type of `out` (ops.dwconv_bn_fwd / dwconv_bn_bwd /
# mbconv_dw_bwd_march) selects every pair dwm_types_ok admits.
UNREACHABLE = {}


# ---------------------------------------------------------------------------------------------------------------- geometry mirror
Geom = collections.namedtuple("Geom", "bands bw last_bw chunks rpc unit rows steps last_steps blocks")


def same_pad(H, K, S):
    Ho = (H + S - 1) // S
    return Ho, max((Ho - 1) * S + K - H, 0) // 2


def march_split(N, cgs, P, Q, unit, bmax, ts, bwd):
    bands = -(-Q // bmax)
    bw = -(-(-(-Q // bands)) // ts) * ts          # balanced bands, whole strips
    bands = -(-Q // bw)
    chunks = (TARGET_BWD if bwd else TARGET_FWD) // (N * cgs * bands)
    chunks = max(min(chunks, (P + 2 * unit - 1) // (2 * unit)), 1)     # at least two steps per chunk
    rpc = -(-(-(-P // chunks)) // unit) * unit
    chunks = -(-P // rpc)
    last = P - (chunks - 1) * rpc
    return Geom(bands, bw, Q - (bands - 1) * bw, chunks, rpc, unit, P, rpc // unit, -(-last // unit), N * bands * chunks)


def geom_fwd(N, H, W, C, K, S):
    (Ho, _), (Wo, _) = same_pad(H, K, S), same_pad(W, K, S)
    return march_split(N, -(-C // 32), Ho, Wo, 4, 28 if S == 1 else 14, 4 if S == 1 else 2, False)


def geom_bwd(N, H, W, C, K, S):
    """Backward: tiles over the layer's INPUT; at stride 2 in 2 x 2 patches of padded coordinates (rows, bw, rpc in pairs, a step = 2)."""
    if S == 1:
        return march_split(N, -(-C // 32), H, W, 4, 28, 4, True)
    (_, pt), (_, pl) = same_pad(H, K, S), same_pad(W, K, S)
    py, px = ((H + pt - 1) >> 1) - (pt >> 1) + 1, ((W + pl - 1) >> 1) - (pl >> 1) + 1
    return march_split(N, -(-C // 32), py, px, 2, 14, 1, True)


def geom(inst, shape):
    N, H, W, C = shape
    return (geom_fwd if inst.entry == "fwd" else geom_bwd)(N, H, W, C, inst.k, inst.s)


# ---------------------------------------------------------------------------------------------------------------- shapes
# stride -> kind -> (N, H, W, C) of the depthwise conv's INPUT.
#   edge: two bands, C = 36 (a second channel group of 4 channels), 9 images (the fused backward sums stage 1 in groups of 8 + 1), two
#         steps per chunk, two or three chunks; the stride-2 forward's last chunk is a single step.
#   long: N * ceil(C / 32) * bands = 15 * 8 * 2 = 240, so one chunk per (image, band): 7 steps at stride 1 in both directions, 5
#         forward / 9 backward at stride 2; a last channel group of 28; image groups 8 + 7.
SHAPES = {
    1: {"edge": (9, 13, 33, 36), "long": (15, 26, 33, 252)},
    2: {"edge": (9, 21, 35, 36), "long": (15, 35, 33, 252)},
}
# The stride-2 BACKWARD tiles 2 x 2 patches: W = 35 gives 18 patch columns = two bands of 9 (no narrower last band) and H = 35 gives 18
# patch rows = 9 whole steps (no partial last step).  Its instances get the two properties from a companion of each shape: W = 33 ->
# 17 patch columns (9 + 8), H = 33 -> 17 patch rows (8 steps + a half one); the forward of these would be 9 + 8 columns, 5 steps too.
S2_BWD_COMPANIONS = {"edge": (9, 21, 33, 36), "long": (15, 33, 33, 252)}
MIN_STEPS = {("fwd", 1): 7, ("fwd", 2): 5, ("bwd", 1): 7, ("bwd", 2): 7}      # of a long case, per (direction, stride)

Case = collections.namedtuple("Case", "inst kind shape")


def cases():
    out = []
    for i in INSTANCES:
        if i in UNREACHABLE:
            continue
        for kind in ("edge", "long"):
            out.append(Case(i, kind, SHAPES[i.s][kind]))
            if i.entry != "fwd" and i.s == 2:
                out.append(Case(i, kind, S2_BWD_COMPANIONS[kind]))
    return out


def case_id(c):
    i = c.inst
    return "{}-k{}s{}-{}-{}_{}-{}-{}".format(i.entry, i.k, i.s, "bn" if i.bn else "plain", i.ta, i.tb, c.kind, "x".join(map(str, c.shape)))


def target_overridden():
    return os.environ.get(ENV_TARGET) is not None


# ---------------------------------------------------------------------------------------------------------------- float64 references
EPS, MOM = 1e-3, 0.99


def _torch():
    import torch
    return torch


def rnd(*shape, seed=0, scale=1.0):
    torch = _torch()
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def stored(t, ty):
    """float64 tensor holding exactly the values a device tensor of storage type ty will hold (round to nearest even)."""
    torch = _torch()
    t = t.float()
    return (t.to(torch.bfloat16).float() if ty == "bf16" else t).double()


def swish_grad(u):
    sg = _torch().sigmoid(u)
    return sg * (1.0 + u * (1.0 - sg))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def batch_stats(z):
    """(mean, biased variance, rstd) over (N, H, W) in float64."""
    torch = _torch()
    mean, var = z.mean(dim=(0, 1, 2)), z.var(dim=(0, 1, 2), unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def conv_with_grads(a, w, s, dy_of):
    """y = depthwise SAME conv of a [N,H,W,C] with w [k,k,C,1] (oracle.efficientlab_ref.conv2d_same), and the gradients of
    sum(y * dy) w.r.t. a and w through autograd.  dy_of(y_shape_nhwc) -> dy [N,Ho,Wo,C] or None (forward only)."""
    torch = _torch()
    from oracle import efficientlab_ref as R
    al, wl = a.detach().requires_grad_(True), w.detach().requires_grad_(True)
    y = R.conv2d_same(_nchw(al), wl, s, groups=a.shape[-1])
    dy = dy_of(tuple(_nhwc(y.detach()).shape))
    if dy is None:
        return _nhwc(y.detach()), None, None
    ga, gw = torch.autograd.grad(y, [al, wl], _nchw(dy))
    return _nhwc(y.detach()), ga.detach(), gw.detach()


def bn_swish(z, mean, rstd, gamma, beta):
    """(a, u, xhat) of a = swish(gamma xhat + beta)."""
    torch = _torch()
    xhat = (z - mean) * rstd
    u = xhat * gamma + beta
    return u * torch.sigmoid(u), u, xhat


def fused_dz1(da2, z1, mean1, rstd1, gamma1, beta1, gate, chan_add):
    """The depthwise batch norm's backward as mliis_mbconv_dw_bwd_march forms it on load, float64 end to end:
    g = (da2 gate + chan_add) swish'(gamma1 xhat1 + beta1); stage1 [N,2,C] = per-image {sum g, sum g xhat1}, handed to the device as
    fp32 -- the means of dz1 = gamma1 rstd1 (g - mean g - xhat1 mean(g xhat1)) and dgamma1 / dbeta1 come from those fp32 values."""
    torch = _torch()
    xh = (z1 - mean1) * rstd1
    g = (da2 * gate[:, None, None, :] + chan_add[:, None, None, :]) * swish_grad(xh * gamma1 + beta1)
    stage1 = torch.stack([g.sum(dim=(1, 2)), (g * xh).sum(dim=(1, 2))], dim=1).float()
    tot = stage1.double().sum(0)
    rows = z1.shape[0] * z1.shape[1] * z1.shape[2]
    dz1 = gamma1 * rstd1 * (g - tot[0] / rows - xh * (tot[1] / rows))
    return dz1, stage1, tot[1], tot[0]     # dgamma1 = sum g xhat1, dbeta1 = sum g
