"""Saving evaluation predictions: every test image's predicted mask as a PNG, optionally the query image tinted where the mask is set
(the reference's SAVE_PREDICTIONS switch: supervised_reptile/reptile.py:495-513 through utils/viz.py:48-85, which renders with
matplotlib).  No third-party dependency: the two PNG flavours needed are written (and, for the tests, read back) here with zlib."""
from __future__ import annotations

import os
import re
import struct
import zlib

import numpy as np

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_GREY, _RGB = 0, 2   # PNG colour types


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, array) -> None:
    """bool [H,W] -> 1-bit greyscale PNG (foreground white; rows packed most-significant bit first and padded to a byte);
    uint8 [H,W,3] -> 8-bit RGB PNG.  Filter type 0 on every row, one IDAT chunk."""
    a = np.asarray(array)
    if a.dtype == np.bool_ and a.ndim == 2:
        depth, colour, rows = 1, _GREY, np.packbits(a, axis=1, bitorder="big")
    elif a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        depth, colour, rows = 8, _RGB, np.ascontiguousarray(a).reshape(a.shape[0], -1)
    else:
        raise ValueError("write_png: expected a bool [H,W] or uint8 [H,W,3] array, got {} {}".format(a.dtype, a.shape))
    H, W = a.shape[:2]
    if H == 0 or W == 0:
        raise ValueError("write_png: empty image")
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rows], axis=1).tobytes()   # filter byte 0 in front of every row
    ihdr = struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))


def png_chunks(data: bytes):
    """[(type, payload)] of a PNG byte string; the signature and every chunk's CRC are verified."""
    if data[:8] != PNG_SIGNATURE:
        raise ValueError("not a PNG file")
    out, pos = [], 8
    while pos < len(data):
        (n,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        payload = data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if len(payload) != n or crc != (zlib.crc32(kind + payload) & 0xFFFFFFFF):
            raise ValueError("PNG chunk {!r}: bad length or CRC".format(kind))
        out.append((kind, payload))
        pos += 12 + n
    if not out or out[0][0] != b"IHDR" or out[-1][0] != b"IEND":
        raise ValueError("PNG without IHDR / IEND")
    return out


def read_png(path) -> np.ndarray:
    """What write_png writes, back: bool [H,W] of a 1-bit greyscale file, uint8 [H,W,3] of an 8-bit RGB one (filter type 0 only)."""
    with open(path, "rb") as f:
        chunks = png_chunks(f.read())
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if (depth, colour) not in ((1, _GREY), (8, _RGB)) or comp or filt or lace:
        raise ValueError("read_png reads the files of write_png only (1-bit greyscale / 8-bit RGB, not interlaced)")
    raw = zlib.decompress(b"".join(p for k, p in chunks if k == b"IDAT"))
    stride = (W + 7) // 8 if depth == 1 else 3 * W
    rows = np.frombuffer(raw, np.uint8)
    if rows.size != H * (stride + 1):
        raise ValueError("PNG data of the wrong size")
    rows = rows.reshape(H, stride + 1)
    if rows[:, 0].any():
        raise ValueError("read_png reads filter type 0 only")
    if depth == 1:
        return np.unpackbits(rows[:, 1:], axis=1, bitorder="big")[:, :W].astype(bool)
    return rows[:, 1:].reshape(H, W, 3).copy()


def overlay(image, mask, tint=(255, 128, 0), alpha=0.5) -> np.ndarray:
    """uint8 [H,W,3]: `image` ([H,W,3], values on the 0..255 scale) with the pixels of `mask` (bool [H,W]) blended towards `tint`:
    foreground (1 - alpha) * image + alpha * tint, background the image; computed in float32, rounded half to even, clipped to 0..255.
    This is this project's own definition of the picture -- it is NOT pixel-identical to the matplotlib rendering of the reference
    (utils/viz.py)."""
    img, m = np.asarray(image, dtype=np.float32), np.asarray(mask).astype(bool)
    if img.ndim != 3 or img.shape[2] != 3 or m.shape != img.shape[:2]:
        raise ValueError("overlay: expected image [H,W,3] and mask [H,W], got {} / {}".format(img.shape, m.shape))
    a = np.float32(alpha)
    fg = (np.float32(1.0) - a) * img + a * np.asarray(tint, dtype=np.float32)
    out = np.where(m[..., None], fg, img)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


class PredictionWriter:
    """<directory>/<task>/sample<k>_query<j>_mask.png (and ..._overlay.png with overlays=True and an image): k = the evaluation pass
    (eval_sample_num, 0 when None), j = the position of the image among the task's test images."""

    def __init__(self, directory, overlays: bool = False):
        self.directory, self.overlays = str(directory), bool(overlays)

    @staticmethod
    def _task_dir(task_name) -> str:
        name = re.sub(r"[\\/]+", "_", str(task_name)).strip()
        if os.sep not in "\\/":
            name = name.replace(os.sep, "_")
        return "_" if name in ("", ".", "..") else name

    def save(self, task_name, sample_num, j, mask, image=None):
        d = os.path.join(self.directory, self._task_dir(task_name))
        os.makedirs(d, exist_ok=True)
        stem = os.path.join(d, "sample{}_query{}".format(0 if sample_num is None else int(sample_num), int(j)))
        m = np.asarray(mask).astype(bool)
        write_png(stem + "_mask.png", m)
        if self.overlays and image is not None:
            write_png(stem + "_overlay.png", overlay(image, m))
