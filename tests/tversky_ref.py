"""The Tversky region term of the inner loop's loss (include/mliis_region.h, csrc/tversky.hip) on the host: its float64 torch reference
(autograd for gradients), a numpy mirror of the closed-form gradient the kernels implement, and the cases test_tversky_cpu.py and
test_tversky_gpu.py share.

For image n, with p1 the channel-1 softmax and y1 the stored, unsmoothed foreground label:

    I = sum p1 y1,  Sp = sum p1,  St = sum y1,  D_n = I + alpha (Sp - I) + beta (St - I) + eps,  T_n = (I + eps) / D_n,  eps = 1e-7
    T = mean_n T_n,   loss = L_pix - ln(2 T / (T + 1)) + extra_loss

L_pix is tests/focal_ref.py's pixel term (gamma = 0, W = 1: the cross-entropy); the soft IoU the entry points report in out[2] is its
soft_iou, whatever alpha and beta are.  The inputs are focal_ref's makers at focal_ref's shapes (tests/head_instances.py's: three fold
rounds of 8 images, 33 partial blocks, the 256-block cap, the fused head at its predicate's limit and just past it).  The pairs
(1, 1), (1/2, 1/2), (0.3, 0.7), (0.7, 0.3), (0, 1), (1, 0) and (2, 0.25) -- the last with a negative (1 - alpha - beta) -- each appear
under both entry points; (0.3, 0.7) also with (gamma, W) = (2, 4) and ls = 0.1.  In two head shapes the mask batch image 0 reads is made
empty in one variant and full in another: there eps carries T_n.  (Labels that are empty in EVERY image with alpha = 0 leave eps the whole
denominator, which is ill-conditioned in this reference itself: not a case.)

This file imports neither the package nor the library; references are computed once per case and never written."""
import collections
import functools

import numpy as np
import torch

import focal_ref as FR

EXTRA = FR.EXTRA
EPS = 1e-7
PAIRS = ((1.0, 1.0), (0.5, 0.5), (0.3, 0.7), (0.7, 0.3), (0.0, 1.0), (1.0, 0.0), (2.0, 0.25))


# ---------------------------------------------------------------------------------------------------------------- the definition
def tversky_index(logits, labels, alpha, beta):
    """T: the batch mean of the images' Tversky indices, float64 torch, differentiable."""
    p1, y1 = torch.softmax(logits, dim=-1)[..., 1].flatten(1), labels[..., 1].flatten(1)
    inter = (p1 * y1).sum(1)
    sp, st = p1.sum(1), y1.sum(1)
    return ((inter + EPS) / (inter + alpha * (sp - inter) + beta * (st - inter) + EPS)).mean()


def region_term(logits, labels, alpha, beta):
    t = tversky_index(logits, labels, alpha, beta)
    return -torch.log(2 * t / (t + 1))


def loss_terms(logits, labels, ls, gamma, fg_weight, alpha, beta):
    """(loss, L_pix, iou): what the entry points leave in out[0..2], before extra_loss."""
    pix = FR.pixel_term(logits, labels, ls, gamma, fg_weight)
    return pix + region_term(logits, labels, alpha, beta), pix.detach(), FR.soft_iou(logits, labels).detach()


def region_grad_mirror(z, y, alpha, beta):
    """d(region term)/dz by the closed form of include/mliis_region.h, numpy float64 [N,H,W,2]:
    dp1 = (A_n y1 - B_n (alpha + (1 - alpha - beta) y1)) p1 (1 - p1), A_n = (1 / D_n) (dL/dT) / N, B_n = ((I + eps) / D_n^2) (dL/dT) / N,
    dL/dT = -1 / (T (T + 1)); the gradient w.r.t. z0 is the negative."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = z.shape[0]
    m = z.max(-1)
    e0, e1 = np.exp(z[..., 0] - m), np.exp(z[..., 1] - m)
    p1 = e1 / (e0 + e1)
    y1 = y[..., 1]
    ax = tuple(range(1, z.ndim - 1))
    I, Sp, St = (p1 * y1).sum(ax), p1.sum(ax), y1.sum(ax)
    D = I + alpha * (Sp - I) + beta * (St - I) + EPS
    T = ((I + EPS) / D).mean()
    dLdT = -1.0 / (T * (T + 1.0))
    A, B = (1.0 / D) * dLdT / N, ((I + EPS) / D ** 2) * dLdT / N
    shape = (N,) + (1,) * len(ax)
    d1 = (A.reshape(shape) * y1 - B.reshape(shape) * (alpha + (1.0 - alpha - beta) * y1)) * p1 * (1.0 - p1)
    return np.stack([-d1, d1], -1)


# ---------------------------------------------------------------------------------------------------------------- cases
# entry: tversky_ce | head.  inst: the launches behind the case ("refused": nothing is launched).
Case = collections.namedtuple("Case", "entry name inst why p")

CHAIN, CHAIN_NOGRAD, HEAD = ("partial", "fold", "grad"), ("partial", "fold"), ("sums", "fold", "tiles")


def _ce(name, why, N, S, H, W, ab, grad=1, gamma=0.0, fgw=1.0, ls=0.0, idx=True, extra=0.0, zscale=3.0):
    return Case("tversky_ce", name, CHAIN if grad else CHAIN_NOGRAD, why,
                dict(N=N, S=S, H=H, W=W, alpha=ab[0], beta=ab[1], grad=grad, gamma=gamma, fgw=fgw, ls=ls, idx=idx, extra=extra, zscale=zscale))


def _head(name, why, shape, ab, gamma=0.0, fgw=1.0, ls=0.0, mask0=None, refused=False):
    """shape: the name of focal_ref's head case whose maps, batch and index vector this case takes."""
    q = FR.case(shape).p
    return Case("head", name, "refused" if refused else HEAD, why,
                dict(N=q["N"], S=q["S"], Hd=q["Hd"], Wd=q["Wd"], H=q["H"], W=q["W"], idx=q["idx"], alpha=ab[0], beta=ab[1], gamma=gamma, fgw=fgw,
                     ls=ls, mask0=mask0))


def cases():
    return [
        _ce("idx9", "9 images through a 4-label index vector; the focal, weighted, smoothed pixel term", 9, 4, 9, 7, (0.3, 0.7), gamma=2.0, fgw=4.0,
            ls=0.1),
        _ce("n17", "N > 16: three fold rounds of 8 images, no index vector; the soft IoU", 17, 17, 16, 12, (1.0, 1.0), idx=False),
        _ce("nblk33", "33 partial blocks: one more than the 32 folding lanes; the soft Dice", 2, 2, 257, 257, (0.5, 0.5), ls=0.1),
        _ce("nblk256", "the 256-block cap: the partial kernel grid-strides", 1, 1, 725, 725, (0.7, 0.3), gamma=0.5),
        _ce("saturated", "logits scaled by 30: |z0 - z1| up to ~180; false alarms cost nothing", 9, 4, 9, 7, (0.0, 1.0), gamma=0.5, fgw=4.0,
            zscale=90.0),
        _ce("nograd", "no gradient: partial sums and the fold; misses cost nothing", 9, 4, 9, 7, (1.0, 0.0), grad=0, ls=0.1),
        _ce("extra-loss", "extra_loss is added to out[0] only; alpha + beta > 1", 9, 4, 9, 7, (2.0, 0.25), extra=EXTRA),
        _head("limit", "both axes at the predicate's limit; the focal, weighted, smoothed pixel term", "limit", (0.3, 0.7), gamma=2.0, fgw=4.0, ls=0.1),
        _head("n9", "N > 8 through an index vector, an odd factor", "n9", (0.5, 0.5), ls=0.1),
        _head("hd2", "Hd = 2: one partial tile, no index vector", "hd2", (0.0, 1.0)),
        _head("mixed-39", "rows down, columns up by the last admitted factor; alpha + beta > 1", "mixed-39", (2.0, 0.25), fgw=0.25),
        _head("identity", "same size; the soft IoU", "identity", (1.0, 1.0)),
        _head("limit-fa", "the limit shape with false alarms weighted up", "limit", (0.7, 0.3)),
        _head("n9-miss-free", "the n9 shape with misses free", "n9", (1.0, 0.0), gamma=0.5),
        _head("limit-empty", "batch image 0 reads an empty mask: T_0 = eps / (alpha Sp + eps)", "limit", (0.3, 0.7), mask0="empty"),
        _head("limit-full", "batch image 0 reads a full mask: no false alarm is possible", "limit", (0.7, 0.3), mask0="full"),
        _head("n9-empty", "the label three batch images read is empty", "n9", (2.0, 0.25), mask0="empty"),
        _head("n9-full", "the label three batch images read is full", "n9", (0.5, 0.5), ls=0.1, mask0="full"),
        _head("refused-square", "the first factor the predicate refuses", "refused-square", (0.3, 0.7), refused=True),
        _head("mixed-40", "columns up by 39/8: the predicate refuses the column factor", "mixed-40", (0.3, 0.7), refused=True),
    ]


def cases_of(entry):
    return [c for c in cases() if c.entry == entry]


def case_id(c):
    return c.name


def case(name):
    return {c.name: c for c in cases()}[name]


# ---------------------------------------------------------------------------------------------------------------- inputs and references
def _scalars(p):
    return tuple(FR.as_f32(p[k]) for k in ("ls", "gamma", "fgw", "alpha", "beta"))


@functools.lru_cache(maxsize=None)
def ce_oracle(name):
    p = case(name).p
    N, S, H, W = p["N"], p["S"], p["H"], p["W"]
    z = FR.fp32_exact(FR.rnd(N, H, W, 2, seed=40) * p["zscale"])
    labels = FR.make_labels(S, H, W, 41, True)
    idx = FR.make_index(N, S, p["idx"])
    used = labels[idx] if idx else labels[:N]
    ls, gamma, fgw, alpha, beta = _scalars(p)
    zr = z.clone().requires_grad_(True)
    loss, pix, iou = loss_terms(zr, used, ls, gamma, fgw, alpha, beta)
    (gz,) = torch.autograd.grad(loss, [zr], retain_graph=True)
    (greg,) = torch.autograd.grad(region_term(zr, used, alpha, beta), [zr])
    return dict(z=z, labels=labels, idx=idx, used=used, loss=loss.item() + p["extra"], pix=pix.item(), iou=iou.item(), gz=gz, greg=greg)


@functools.lru_cache(maxsize=None)
def head_oracle(name):
    p = case(name).p
    N, S, Hd, Wd, H, W = p["N"], p["S"], p["Hd"], p["Wd"], p["H"], p["W"]
    small = FR.fp32_exact(FR.rnd(N, Hd, Wd, 2, seed=90) * 3)
    labels = FR.make_labels(S, H, W, 91, False).clone()
    idx = FR.make_index(N, S, p["idx"])
    if p["mask0"] is not None:      # the label batch image 0 reads
        m = 0.0 if p["mask0"] == "empty" else 1.0
        labels[idx[0] if idx else 0] = torch.tensor([1.0 - m, m], dtype=torch.float64)
    used = labels[idx] if idx else labels[:N]
    assert sum(1 for n in range(N) if 0 < used[n, ..., 1].sum().item() < H * W) >= 1 and N >= 2      # a non-degenerate image remains
    ls, gamma, fgw, alpha, beta = _scalars(p)
    sm = small.clone().requires_grad_(True)
    logits = FR.resize(sm, H, W)
    loss, pix, iou = loss_terms(logits, used, ls, gamma, fgw, alpha, beta)
    (gs,) = torch.autograd.grad(loss, [sm], retain_graph=True)
    (greg,) = torch.autograd.grad(region_term(logits, used, alpha, beta), [logits])
    return dict(small=small, labels=labels, idx=idx, used=used, logits=logits.detach(), loss=loss.item() + EXTRA, pix=pix.item(), iou=iou.item(),
                gs=gs, greg=greg)
