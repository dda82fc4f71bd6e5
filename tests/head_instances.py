"""The decoder tail's launch paths (csrc/head.hip: 13 kernels behind resize forward / backward, the final 1x1 conv, softmax cross-entropy
with the dice term, the fused head, DARC1 and the ASPP swish-mask) as a pure mirror of the routing its entry points do, and the cases
that reach every route and launch form.  Shared by test_head_instances_cpu.py (the mirror against the source and the library's host-only
queries: no GPU) and test_head_instances_gpu.py (float64 parity per case).

The launchers choose by channel count, leading dimensions and pointer alignment (the 4-float or the 2-float resize kernels), by C, Wo and
the float32 comparison 2/sh + 3 > 4 (the separable resize transpose and its row batch), by (dice, gradient, mask) (two or three launches
of the loss), and by a float32 predicate on the two maps (whether the fused head takes them at all).  Everything that decides in float32
is computed in numpy.float32 here, spelled as the source spells it.

This file imports neither torch nor the library."""
import collections

import numpy as np

F32 = np.float32

EW_MAX_BLOCKS = 4096        # ew_blocks: element-wise launches are capped, the kernels grid-stride
CE_PIXELS_PER_BLOCK = 256 * 8
CE_MAX_BLOCKS = 256         # ce_partial_k: at most 256 partial blocks per image
CE_FOLD_IMAGES, CE_FOLD_LANES = 8, 32      # ce_finalize: 8 images per round, 32 lanes fold an image's blocks
DARC1_MAX_BLOCKS = 1024
HEAD_TILE, HEAD_FOOT = 8, 48               # kHeadTile, kHeadFoot
ROWS_MIN_C, ROWS_MAX_WO, ROWS_THREADS = 16, 512, 512      # the separable resize transpose: C >= 16 && Wo <= 512, 512 threads


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------- float32 geometry
def scale(n_in, n_out):
    """(float)(in - 1) / (float)(out - 1)"""
    return F32(n_in - 1) / F32(n_out - 1)


def src_coord(o, s, n_in):
    """src_coord of common.hpp: (i0, i1) of output coordinate(s) o (the weight is not needed here)."""
    f = np.asarray(o, dtype=F32) * F32(s)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1)


def head_lo(i, s):
    """(int)floorf((float)(i - 1) / s) - 1, clamped at 0: first candidate output row / column of input row / column i"""
    v = np.floor(np.asarray(np.asarray(i) - 1, dtype=F32) / F32(s)).astype(np.int64) - 1
    return np.maximum(v, 0)


def head_hi(i, s, n):
    """(int)ceilf((float)(i + 1) / s) + 1, clamped at n - 1"""
    v = np.ceil(np.asarray(np.asarray(i) + 1, dtype=F32) / F32(s)).astype(np.int64) + 1
    return np.minimum(v, n - 1)


def candidates(i, n_in, n_out):
    """(lo, hi) of the candidate range the transpose kernels walk for input coordinate i (resize_bwd_k, resize_bwd_rows_k and
    head_ce_fused_k spell the same two formulas)."""
    s = scale(n_in, n_out)
    return int(head_lo(i, s)), int(head_hi(i, s, n_out))


def head_tiles(n):
    return cdiv(n, HEAD_TILE)


def head_supported(Hd, Wd, H, W):
    """mliis_head_ce_fused_supported"""
    if Hd <= 1 or Wd <= 1 or H <= 1 or W <= 1:
        return False
    sh, sw = scale(Hd, H), scale(Wd, W)
    fh = int(np.ceil(F32(HEAD_TILE + 1) / sh)) + 5
    fw = int(np.ceil(F32(HEAD_TILE + 1) / sw)) + 5
    return fh <= HEAD_FOOT and fw <= HEAD_FOOT


def head_footprint(Hd, H):
    """The largest FH = fo1 - fo0 + 1 over the tiles of one axis, as head_ce_fused_k computes it."""
    s = scale(Hd, H)
    hi0 = np.arange(head_tiles(Hd)) * HEAD_TILE
    hi1 = np.minimum(hi0 + HEAD_TILE - 1, Hd - 1)
    return int((head_hi(hi1, s, H) - head_lo(hi0, s) + 1).max())


def head_uncovered(Hd, H):
    """Image rows that lie outside the candidate range of one of their two source rows (the transpose would miss them)."""
    s = scale(Hd, H)
    ho = np.arange(H)
    bad = np.zeros(H, dtype=bool)
    for y in src_coord(ho, s, Hd):
        bad |= (ho < head_lo(y, s)) | (ho > head_hi(y, s, H))
    return int(bad.sum())


# ---------------------------------------------------------------------------------------------------------------- routing mirror
def ew_blocks(q):
    return int(min(max(cdiv(q, 256), 1), EW_MAX_BLOCKS))


def route_resize_fwd(C, ldx, ldy, aligned16):
    if C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and aligned16:
        return "resize_fwd_k<4>"
    return "resize_fwd_k<2>"


def route_resize_bwd(N, Hi, Wi, Ho, Wo, C, lddy, lddx, aligned16):
    if C % 4 == 0 and lddx % 4 == 0 and lddy % 4 == 0 and aligned16:
        if C >= ROWS_MIN_C and Wo <= ROWS_MAX_WO and Hi <= 65535 and N <= 65535:
            sh = scale(Hi, Ho)
            return "resize_bwd_rows_k<12>" if F32(2) / sh + F32(3) > F32(4) else "resize_bwd_rows_k<4>"
        return "resize_bwd_k<4>"
    return "resize_bwd_k<2>"


def rows_lds_bytes(Wo):
    return Wo * 8 * 16


def softmax_ce_nblk(H, W):
    return min(cdiv(H * W, CE_PIXELS_PER_BLOCK), CE_MAX_BLOCKS)


def softmax_ce_launches(dice, grad, pred):
    if not dice and (grad or pred):
        return ("ce_partial_k", "ce_grad_k+fin")
    if grad or pred:
        return ("ce_partial_k", "ce_finalize_k", "ce_grad_k")
    return ("ce_partial_k", "ce_finalize_k")


def softmax_ce_workspace_floats(N, H, W):
    if N <= 0 or H <= 0 or W <= 0:
        return 0
    return N * softmax_ce_nblk(H, W) * 4 + 2 * N + 8


def head_workspace_floats(N, Hd, Wd):
    if N <= 0 or Hd <= 0 or Wd <= 0:
        return 0
    return N * head_tiles(Hd) * head_tiles(Wd) * 4 + 2 * N + 8


def darc1_nblk(per_img):
    return min(cdiv(per_img, 256), DARC1_MAX_BLOCKS)


# every launch form a case must reach: the six resize instances, the three forms of the loss, the fused head in its two forms and its
# refusal, and the single-kernel entry points
ROUTES = ("resize_fwd_k<4>", "resize_fwd_k<2>", "resize_bwd_rows_k<12>", "resize_bwd_rows_k<4>", "resize_bwd_k<4>", "resize_bwd_k<2>",
          "final_conv", ("ce_partial_k", "ce_grad_k+fin"), ("ce_partial_k", "ce_finalize_k", "ce_grad_k"), ("ce_partial_k", "ce_finalize_k"),
          "head", "head-refused", "darc1", "swish_mask")

# hipLaunchKernelGGL names of head.hip behind each route
KERNELS = {
    "final_conv": ("final_conv_fwd_k", "final_conv_bwd_data_k"),
    "head": ("head_ce_fused_k", "ce_finalize_k", "final_conv_bwd_data_k"),
    "head-refused": (),
    "darc1": ("darc1_partial_k", "darc1_apply_k"),
    "swish_mask": ("swish_mask_fwd_k", "swish_mask_bwd_k"),
}


def kernels_of(inst):
    if isinstance(inst, tuple):
        return tuple(k.split("+")[0] for k in inst)
    return KERNELS.get(inst, (inst,))


# ---------------------------------------------------------------------------------------------------------------- cases
# entry: resize_fwd | resize_bwd | final_conv | softmax_ce | head | darc1 | swish_mask.  p: the shape and options of the case.
Case = collections.namedtuple("Case", "entry name inst why p")

SLICE = (2, 10, 12)      # [..., 2:10] of a tensor of leading dimension 12: C = 8, pointer 8-byte but not 16-byte aligned


def _resize(N, Hi, Wi, Ho, Wo, C, sliced=False):
    return dict(N=N, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, C=C, sliced=sliced)


def resize_lds(p, out_pad):
    """(ld of the gradient / input, ld of the target / output, both pointers 16-byte aligned) of a resize case.  A sliced case is
    SLICE on both sides; every backward case writes [..., out_pad:out_pad + C] of a tensor out_pad * 2 wider."""
    if p["sliced"]:
        return SLICE[2], SLICE[2], (SLICE[0] * 4) % 16 == 0
    return p["C"], p["C"] + 2 * out_pad, (out_pad * 4) % 16 == 0


BWD_PAD = 4      # the backward cases' target: channels [4, 4 + C) of C + 8


def _fwd(name, why, **kw):
    p = _resize(**kw)
    ldx, ldy, al = resize_lds(p, 0)
    return Case("resize_fwd", name, route_resize_fwd(p["C"], ldx, ldy, al), why, p)


def _bwd(name, why, **kw):
    p = _resize(**kw)
    lddy, lddx, al = resize_lds(p, BWD_PAD)
    return Case("resize_bwd", name, route_resize_bwd(p["N"], p["Hi"], p["Wi"], p["Ho"], p["Wo"], p["C"], lddy, lddx, al), why, p)


def _ce(name, why, N, S, H, W, dice, grad, pred, idx=True, ls=0.0, extra=0.0, zscale=3.0, ties=0.0):
    p = dict(N=N, S=S, H=H, W=W, dice=dice, grad=grad, pred=pred, idx=idx, ls=ls, extra=extra, zscale=zscale, ties=ties)
    return Case("softmax_ce", name, softmax_ce_launches(dice, grad, pred), why, p)


def _head(name, why, N, S, Hd, Wd, H, W, ls=0.0, idx=True):
    p = dict(N=N, S=S, Hd=Hd, Wd=Wd, H=H, W=W, ls=ls, idx=idx)
    return Case("head", name, "head" if head_supported(Hd, Wd, H, W) else "head-refused", why, p)


def _darc1(name, why, N, H, W, plant, zero=False, outs="both", weight=0.5):
    """plant: flat positions (of H * W * 2) that all get the winning column; the first of them must win."""
    return Case("darc1", name, "darc1", why, dict(N=N, H=H, W=W, plant=tuple(plant), zero=zero, outs=outs, weight=weight))


BIG = 363 * 363 * 2      # per_img 263 538 > 1024 * 256


def cases():
    out = [
        # ---- resize forward
        _fwd("fwd4-dense", "4-float path", N=2, Hi=7, Wi=5, Ho=20, Wo=13, C=8),
        _fwd("fwd2-misaligned-slice", "C % 4 == 0 but the views are only 8-byte aligned", N=2, Hi=7, Wi=5, Ho=20, Wo=13, C=8, sliced=True),
        _fwd("fwd4-hi1", "Hi = 1: both source rows are row 0", N=2, Hi=1, Wi=1, Ho=9, Wo=7, C=4),
        _fwd("fwd2-mixed", "one axis up-samples, the other down-samples", N=2, Hi=9, Wi=20, Ho=20, Wo=9, C=6),
        _fwd("fwd4-identity", "same size: every weight is 0 or 1", N=2, Hi=4, Wi=4, Ho=4, Wo=4, C=8),
        _fwd("fwd4-grid-stride", "more quads than 4096 * 256: the loop iterates twice", N=3, Hi=48, Wi=48, Ho=192, Wo=192, C=40),
        # ---- resize backward (each in overwrite and accumulate form, into a slice of a sentinel-filled tensor)
        _bwd("rows12-rounds", "about 60 candidate rows: several rounds of 12, and a partial 32-channel group", N=2, Hi=3, Wi=5, Ho=64, Wo=130, C=36),
        _bwd("rows12-lds64k", "Wo = 512: a 64 KiB dynamic LDS launch", N=2, Hi=3, Wi=5, Ho=4, Wo=512, C=16),
        _bwd("bwd4-wo513", "Wo = 513: falls back to the gather form", N=2, Hi=3, Wi=5, Ho=4, Wo=513, C=16),
        _bwd("rows4-down", "down-sampling: four candidate rows at a time", N=2, Hi=28, Wi=28, Ho=14, Wo=14, C=16),
        _bwd("rows4-mixed", "rows down, columns up, a partial 32-channel group", N=2, Hi=20, Wi=9, Ho=9, Wo=40, C=20),
        _bwd("bwd4-narrow", "below 16 channels", N=2, Hi=7, Wi=5, Ho=20, Wo=13, C=12),
        _bwd("bwd2-c2", "C = 2", N=2, Hi=7, Wi=5, Ho=20, Wo=13, C=2),
        _bwd("bwd2-misaligned-slice", "C % 4 == 0 but the views are only 8-byte aligned", N=2, Hi=7, Wi=5, Ho=20, Wo=13, C=8, sliced=True),
        # ---- final conv: x = [..., off:off + C] of leading dimension ld, the mask has the layout of x
        Case("final_conv", "c4", "final_conv", "C = 4: three of the four lanes of a pixel idle", dict(rows=67, C=4, ld=4, off=0, mask=False)),
        Case("final_conv", "slice-mask", "final_conv", "x and the mask are channel slices: ldx > C", dict(rows=77, C=136, ld=152, off=8, mask=True)),
        Case("final_conv", "grid-stride", "final_conv", "more quads than 4096 * 256 in the backward", dict(rows=40000, C=112, ld=116, off=4, mask=False)),
        # ---- softmax cross-entropy: the six (dice, grad, pred) forms
        _ce("form-010", "merged, gradient only", 9, 4, 9, 7, 0, 1, 0),
        _ce("form-001", "merged, mask only (evaluation)", 9, 4, 9, 7, 0, 0, 1),
        _ce("form-011", "merged, gradient and mask", 9, 4, 9, 7, 0, 1, 1, ls=0.1),
        _ce("form-111", "dice: three launches", 9, 4, 9, 7, 1, 1, 1, ls=0.1),
        _ce("form-100", "dice, finalize only", 9, 4, 9, 7, 1, 0, 0),
        _ce("form-000", "finalize only", 9, 4, 9, 7, 0, 0, 0),
        _ce("n17", "N > 16: three rounds of 8 images", 17, 17, 16, 12, 1, 1, 1, idx=False),
        _ce("nblk33", "33 partial blocks: one more than the 32 folding lanes", 2, 2, 257, 257, 1, 1, 0),
        _ce("nblk256", "the 256-block cap: ce_partial_k grid-strides", 1, 1, 725, 725, 0, 1, 1),
        _ce("extra-loss", "extra_loss is added to out[0] only", 9, 4, 9, 7, 1, 1, 0, extra=0.375),
        _ce("saturated", "logits scaled by 30: saturated softmax", 9, 4, 9, 7, 1, 1, 1, zscale=90.0),
        _ce("ties", "5 % of the pixels have exactly equal logits", 9, 4, 16, 12, 0, 1, 1, ties=0.05),
        # ---- fused head
        _head("limit", "both axes at the predicate's limit: 47 of 48 footprint rows", 2, 2, 18, 11, 81, 48),
        _head("refused-square", "the first factor the predicate refuses", 2, 2, 11, 11, 49, 49),
        _head("n9", "N > 8, label smoothing, an odd factor", 9, 4, 13, 7, 37, 28, ls=0.1),
        _head("hd2", "Hd = 2: one partial tile", 2, 2, 2, 2, 5, 5, idx=False),
        _head("mixed-40", "rows down, columns up by 39/8: the predicate refuses the column factor", 2, 2, 20, 9, 9, 40),
        _head("mixed-39", "rows down, columns up by the last admitted factor", 2, 2, 20, 9, 9, 39),
        _head("identity", "same size", 2, 2, 21, 21, 21, 21),
        # ---- DARC1
        _darc1("one-block", "one block, the real weight", 1, 3, 5, [17], weight=0.0005),
        _darc1("last-block", "the winner is in the last block", 8, 24, 20, [950]),
        _darc1("stride-second", "the winner is in a thread's second grid-stride pass", 2, 363, 363, [262144 + 700]),
        _darc1("stride-first", "1024-block cap, the winner is in a first pass", 2, 363, 363, [131313]),
        _darc1("tie-thread", "a tie inside one thread's stride", 2, 363, 363, [700, 262144 + 700]),
        _darc1("tie-lanes", "a tie between two lanes of one block", 8, 24, 20, [300, 305]),
        _darc1("tie-blocks", "a tie between two blocks", 8, 24, 20, [100, 100 + 3 * 256]),
        _darc1("tie-apply-thread", "a tie between two blocks that one thread of darc1_apply_k folds", 2, 363, 363, [5 * 256 + 9, (5 + 256) * 256 + 9]),
        _darc1("zero-sign", "one image's logit is exactly 0 at the winner: sign(0) = 0", 8, 24, 20, [511], zero=True),
        _darc1("dlogits-only", "out is null", 8, 24, 20, [256], outs="dlogits"),
        _darc1("out-only", "dlogits is null", 8, 24, 20, [255], outs="out"),
    ]
    # ---- swish-mask: slices [..., 8:152] of leading dimension 152, 30 000 rows
    for pre in (0, 1):
        for mask in (1, 0):
            out.append(Case("swish_mask", "pre{}-{}".format(pre, "mask" if mask else "nomask"), "swish_mask",
                            "more quads than 4096 * 256: the 32-bit loop iterates twice", dict(rows=30000, C=144, ld=152, off=8, pre=pre, mask=mask)))
    return out


def cases_of(entry):
    return [c for c in cases() if c.entry == entry]


def case_id(c):
    return c.name
