"""The focal, foreground-weighted pixel loss (include/mliis_loss.h, csrc/focal.hip) on the host: its float64 torch reference (autograd for
gradients), a numpy mirror of the closed-form gradient the kernels implement, and the cases test_focal_cpu.py and test_focal_gpu.py share.

Per pixel, with (l0, l1) = log_softmax(z), (y0, y1) the stored labels, t_c = y_c (1 - ls) + ls / 2 and w = 1 + (W - 1) y1:

    l = -w (t0 exp(gamma l1) l0 + t1 exp(gamma l0) l1),    L_pix = sum(l) / (N H W)

The dice term and the soft IoU are oracle.efficientlab_ref.loss_fn's, written out (the IoU also when the dice term is off, as the kernels
report it).  Shapes are those of tests/head_instances.py, the smallest that reach each launch form: three fold rounds of 8 images (N = 17),
33 partial blocks (257 x 257), the 256-block cap with a grid-stride (725 x 725), the fused head at its predicate's limit and just past it.
gamma in {0, 0.5, 2, 5}, W in {0.25, 1, 4} and ls in {0, 0.1} are spread over the cases: every value appears with and without the dice
term, and (gamma, W) = (2, 4) in every launch form (gradient with the fold riding, fold only, three launches, the fused head).

This file imports neither the package nor the library; references are computed once per case and never written."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

GAMMAS, WEIGHTS, SMOOTHINGS = (0.0, 0.5, 2.0, 5.0), (0.25, 1.0, 4.0), (0.0, 0.1)
EXTRA = 0.375


# ---------------------------------------------------------------------------------------------------------------- the definition
def pixel_term(logits, labels, ls, gamma, fg_weight):
    """L_pix: float64 torch, differentiable."""
    lp = F.log_softmax(logits, dim=-1)
    l0, l1 = lp[..., 0], lp[..., 1]
    t = labels * (1 - ls) + ls / 2
    w = 1 + (fg_weight - 1) * labels[..., 1]
    per_pixel = -w * (t[..., 0] * torch.exp(gamma * l1) * l0 + t[..., 1] * torch.exp(gamma * l0) * l1)
    return per_pixel.sum() / per_pixel.numel()


def soft_iou(logits, labels):
    p1, t1 = torch.softmax(logits, dim=-1)[..., 1].flatten(1), labels[..., 1].flatten(1)
    inter = (p1 * t1).sum(1)
    return ((inter + 1e-7) / (p1.sum(1) + t1.sum(1) - inter + 1e-7)).mean()


def loss_terms(logits, labels, ls, gamma, fg_weight, dice):
    """(loss, L_pix, iou): what the entry points leave in out[0..2], before extra_loss."""
    pix, iou = pixel_term(logits, labels, ls, gamma, fg_weight), soft_iou(logits, labels)
    loss = pix - torch.log(2 * iou / (iou + 1)) if dice else pix
    return loss, pix.detach(), iou.detach()


def grad_mirror(z, y, ls, gamma, fg_weight):
    """dL_pix/dz by the closed form of include/mliis_loss.h, numpy float64 [N,H,W,2] (everything from the log-softmax; no pow, no 1 - p)."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = z.max(-1)
    lse = m + np.log(np.exp(z[..., 0] - m) + np.exp(z[..., 1] - m))
    l0, l1 = z[..., 0] - lse, z[..., 1] - lse
    p0, p1 = np.exp(l0), np.exp(l1)
    t0, t1 = y[..., 0] * (1 - ls) + ls / 2, y[..., 1] * (1 - ls) + ls / 2
    w = 1 + (fg_weight - 1) * y[..., 1]
    d1 = w * (t1 * (gamma * np.exp(gamma * l0) * p1 * l1 - np.exp((gamma + 1) * l0)) -
              t0 * (gamma * np.exp(gamma * l1) * p0 * l0 - np.exp((gamma + 1) * l1))) / l0.size
    return np.stack([-d1, d1], -1)


# ---------------------------------------------------------------------------------------------------------------- cases
# entry: focal_ce | head.  inst: the launches behind the case ("refused": nothing is launched).
Case = collections.namedtuple("Case", "entry name inst why p")

MERGED, FOLD_ONLY, THREE = ("partial", "grad+fold"), ("partial", "fold"), ("partial", "fold", "grad")


def _ce(name, why, N, S, H, W, dice, grad, gamma, fgw, ls=0.0, idx=True, extra=0.0, zscale=3.0, ties=0.0):
    inst = MERGED if (grad and not dice) else (THREE if grad else FOLD_ONLY)
    return Case("focal_ce", name, inst, why, dict(N=N, S=S, H=H, W=W, dice=dice, grad=grad, gamma=gamma, fgw=fgw, ls=ls, idx=idx, extra=extra,
                                                   zscale=zscale, ties=ties))


def _head(name, why, N, S, Hd, Wd, H, W, gamma, fgw, ls=0.0, idx=True, refused=False):
    return Case("head", name, "refused" if refused else ("head", "fold"), why,
                dict(N=N, S=S, Hd=Hd, Wd=Wd, H=H, W=W, gamma=gamma, fgw=fgw, ls=ls, idx=idx))


def cases():
    return [
        _ce("grad", "no dice term: the fold rides in the gradient launch", 9, 4, 9, 7, 0, 1, 2.0, 4.0),
        _ce("nograd", "no gradient: partial sums and the fold", 9, 4, 9, 7, 0, 0, 2.0, 4.0, ls=0.1),
        _ce("dice", "dice: three launches", 9, 4, 9, 7, 1, 1, 2.0, 4.0, ls=0.1),
        _ce("n17", "N > 16: three rounds of 8 images, no index vector", 17, 17, 16, 12, 1, 1, 5.0, 1.0, idx=False),
        _ce("nblk33", "33 partial blocks: one more than the 32 folding lanes", 2, 2, 257, 257, 1, 1, 0.0, 0.25, ls=0.1),
        _ce("nblk256", "the 256-block cap: the partial kernel grid-strides", 1, 1, 725, 725, 0, 1, 0.5, 0.25),
        _ce("extra-loss", "extra_loss is added to out[0] only", 9, 4, 9, 7, 1, 1, 0.5, 1.0, extra=EXTRA),
        _ce("saturated", "logits scaled by 30: |z0 - z1| up to ~180", 9, 4, 9, 7, 0, 1, 5.0, 4.0, ls=0.1, zscale=90.0),
        _ce("saturated-dice", "the same with the dice term and a fractional exponent", 9, 4, 9, 7, 1, 1, 0.5, 4.0, zscale=90.0),
        _ce("ties", "5 % of the pixels have exactly equal logits; the plain cross-entropy's parameters", 9, 4, 16, 12, 0, 1, 0.0, 1.0, ties=0.05),
        _head("limit", "both axes at the predicate's limit: 47 of 48 footprint rows", 2, 2, 18, 11, 81, 48, 2.0, 4.0),
        _head("n9", "N > 8, label smoothing, an odd factor", 9, 4, 13, 7, 37, 28, 0.5, 0.25, ls=0.1),
        _head("hd2", "Hd = 2: one partial tile, no index vector", 2, 2, 2, 2, 5, 5, 5.0, 1.0, idx=False),
        _head("mixed-39", "rows down, columns up by the last admitted factor", 2, 2, 20, 9, 9, 39, 0.0, 4.0),
        _head("identity", "same size", 2, 2, 21, 21, 21, 21, 2.0, 1.0, ls=0.1),
        _head("refused-square", "the first factor the predicate refuses", 2, 2, 11, 11, 49, 49, 2.0, 4.0, refused=True),
        _head("mixed-40", "columns up by 39/8: the predicate refuses the column factor", 2, 2, 20, 9, 9, 40, 2.0, 4.0, refused=True),
    ]


def cases_of(entry):
    return [c for c in cases() if c.entry == entry]


def case_id(c):
    return c.name


def case(name):
    return {c.name: c for c in cases()}[name]


# ---------------------------------------------------------------------------------------------------------------- inputs and references
def fp32_exact(t):
    return t.float().double()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def make_labels(S, H, W, seed, soft):
    m = torch.rand(S, H, W, generator=torch.Generator().manual_seed(seed)).double()
    m = torch.where(m < 0.6, (m < 0.3).double(), m) if soft else (m > 0.6).double()      # mostly binary, some fractional labels
    return fp32_exact(torch.stack([1 - m, m], -1))


def make_index(N, S, use):
    return [(3 * i + 1) % S for i in range(N)] if use else None


def as_f32(x):
    """A scalar as the C ABI's float sees it (0.1 is not an fp32 number): the references use the value the kernels get."""
    return float(np.float32(x))


def resize(small, H, W):
    """[N,Hd,Wd,2] -> [N,H,W,2], bilinear, align_corners"""
    return F.interpolate(small.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def ce_oracle(name):
    p = case(name).p
    N, S, H, W = p["N"], p["S"], p["H"], p["W"]
    z = fp32_exact(rnd(N, H, W, 2, seed=40) * p["zscale"])
    tied = torch.zeros(N, H, W, dtype=torch.bool)
    if p["ties"]:
        tied = torch.rand(N, H, W, generator=torch.Generator().manual_seed(42)) < p["ties"]
        z[..., 1] = torch.where(tied, z[..., 0], z[..., 1])
        assert abs(tied.double().mean().item() - p["ties"]) < 0.02
    labels = make_labels(S, H, W, 41, True)
    idx = make_index(N, S, p["idx"])
    used = labels[idx] if idx else labels[:N]
    ls, gamma, fgw = as_f32(p["ls"]), as_f32(p["gamma"]), as_f32(p["fgw"])
    zr = z.clone().requires_grad_(True)
    loss, pix, iou = loss_terms(zr, used, ls, gamma, fgw, p["dice"])
    (gz,) = torch.autograd.grad(loss, [zr], retain_graph=True)
    (gpix,) = torch.autograd.grad(pixel_term(zr, used, ls, gamma, fgw), [zr])
    return dict(z=z, labels=labels, idx=idx, used=used, loss=loss.item() + p["extra"], pix=pix.item(), iou=iou.item(), gz=gz, gpix=gpix)


@functools.lru_cache(maxsize=None)
def head_oracle(name):
    p = case(name).p
    N, S, Hd, Wd, H, W = p["N"], p["S"], p["Hd"], p["Wd"], p["H"], p["W"]
    small = fp32_exact(rnd(N, Hd, Wd, 2, seed=90) * 3)
    labels = make_labels(S, H, W, 91, False)
    idx = make_index(N, S, p["idx"])
    used = labels[idx] if idx else labels[:N]
    ls, gamma, fgw = as_f32(p["ls"]), as_f32(p["gamma"]), as_f32(p["fgw"])
    sm = small.clone().requires_grad_(True)
    logits = resize(sm, H, W)
    loss, pix, iou = loss_terms(logits, used, ls, gamma, fgw, False)
    (gs,) = torch.autograd.grad(loss, [sm], retain_graph=True)
    (gpix,) = torch.autograd.grad(loss, [logits])
    return dict(small=small, labels=labels, idx=idx, used=used, logits=logits.detach(), loss=loss.item() + EXTRA, pix=pix.item(), iou=iou.item(),
                gs=gs, gpix=gpix)
