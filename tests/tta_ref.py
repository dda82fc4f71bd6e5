"""Host references of the flip test-time-augmentation tests (a plain module: tests import it, nothing here is collected).

The float64 reference is NOT a restatement of the implementation: it resizes every view's decoder-resolution logits to the image size
(align-corners bilinear, float64), mirrors the FULL-RESOLUTION map of a mirrored view back and averages there; the device merges at decoder
resolution and resizes once.  The two agree because flips commute with the align-corners resize."""
from __future__ import annotations

import numpy as np

FLIPS = {"hflip": (False, True), "vflip": (True, False), "hvflip": (True, True)}      # (rows, columns), restated: not imported from the package
ORDER = ("hflip", "vflip", "hvflip")


def flip_np(z, view):
    """z [N,H,W,C] mirrored as the view says (hflip = np.fliplr of every image)."""
    fr, fc = FLIPS[view]
    z = z[:, ::-1] if fr else z
    return z[:, :, ::-1] if fc else z


def flip_dims(flips):
    """The torch.flip dims of an NHWC tensor for (flip_rows, flip_cols); () for none."""
    return tuple(d for d, f in zip((1, 2), flips) if f)


def _coord(O, I, dt):
    """Source index pair and weight of every output coordinate: scale = (I - 1) / (O - 1), the device's src_coord in dt."""
    scale = dt(dt(I - 1) / dt(O - 1))
    f = (np.arange(O).astype(dt) * scale).astype(dt)
    i0 = np.minimum(np.floor(f).astype(np.int64), I - 1)
    return i0, np.minimum(i0 + 1, I - 1), (f - i0.astype(dt)).astype(dt)


def resize(z, H, W, dt=np.float64):
    """[N,Hd,Wd,C] -> [N,H,W,C], align-corners bilinear in dt.  float64: the reference.  float32: the device's arithmetic restated (fp32
    coordinates and weights, four fused multiply-adds in the order tl, tr, bl, br: a product of two fp32 values is exact in float64, so each
    step is one rounding of the float64 sum to fp32)."""
    z = np.asarray(z, dtype=dt)
    y0, y1, ly = _coord(H, z.shape[1], dt)
    x0, x1, lx = _coord(W, z.shape[2], dt)
    my, mx = (dt(1) - ly).astype(dt), (dt(1) - lx).astype(dt)
    weights = [(my[:, None] * mx[None, :]).astype(dt), (my[:, None] * lx[None, :]).astype(dt), (ly[:, None] * mx[None, :]).astype(dt),
               (ly[:, None] * lx[None, :]).astype(dt)]
    corners = [z[:, y0][:, :, x0], z[:, y0][:, :, x1], z[:, y1][:, :, x0], z[:, y1][:, :, x1]]
    o = np.zeros((z.shape[0], H, W, z.shape[3]), dtype=dt)
    for w, t in zip(weights, corners):
        o = (w[None, :, :, None].astype(np.float64) * t.astype(np.float64) + o.astype(np.float64)).astype(dt)
    return o


def margin_f64(a, views_b, H, W):
    """d = z1 - z0 [N,H,W] in float64 of the mean over the identity view a and the mirrored views {view: b}: every map resized to (H, W)
    first, the mirrored ones flipped back at full resolution."""
    full = [resize(a, H, W)] + [flip_np(resize(b, H, W), v) for v, b in views_b.items()]
    m = sum(full) / float(len(full))
    return m[..., 1] - m[..., 0]


def margin_f32(a, views_b, H, W):
    """The same margin by the device's arithmetic restated in float32 numpy: s = F_v1(b_v1) (+ F_v2(b_v2) ...) in canonical order at decoder
    resolution, merged = (a + s) * fl32(1 / (K + 1)), one resize, z1 - z0."""
    s = None
    for v in ORDER:
        if v in views_b:
            t = flip_np(np.asarray(views_b[v], dtype=np.float32), v)
            s = t if s is None else (s + t).astype(np.float32)
    merged = ((np.asarray(a, dtype=np.float32) + s).astype(np.float32) * np.float32(1.0 / (len(views_b) + 1))).astype(np.float32)
    z = resize(merged, H, W, np.float32)
    return (z[..., 1] - z[..., 0]).astype(np.float32)


def tau_of(*maps):
    """The excluded band of the float64 check: 2^-17 max(1, max |logit|) -- about 16 roundings of at most half an ulp of max |logit| on
    the two sides (2^-20), doubled for the difference (2^-19), times a margin of 4; it also covers the p1 == 0.5 tie of the fp32 softmax."""
    return 2.0 ** -17 * max(1.0, max(float(np.abs(m).max()) for m in maps))
