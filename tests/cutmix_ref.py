"""TEST INFRASTRUCTURE: an independent numpy restatement of the whole mixed batch slk_image_batch_mix builds.

Nothing here is imported from the package under test or from cifar_ref.py: the hash constants are typed in again,
the draws are Python integers, and every output pixel is produced by an explicit loop over (yo, xo) that asks
"which sample shows here, and which of its source pixels is that" — the definition in include/slk.h, not the
kernel's quad gather:

  sample i's pixel at output (c, yo, xo), under i's own draws (dy, dx, flip) and padding pad:
      xs = (flip ? W-1-xo : xo) + dx - pad;  ys = yo + dy - pad
      p  = images[i][c][ys][xs] if 0 <= xs < W and 0 <= ys < H else 0
  the box of batch position s comes from the PRIMARY sample's chain h3..h7 (box_one below);
  inside the applied box the pixel is the partner's, elsewhere the primary's; then ToTensor + Normalize in float32;
  y[s] = a | b << 8 | float32_bits(area / (H W)) << 32, or the plain label a when the box is unapplied or empty.

The numpy twins of loss.pack_mixed / unpack_mixed live here too (pack, unpack)."""
import struct

import numpy as np

M32 = 0xFFFFFFFF
GOLD = 0x9E3779B9


def lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def chain(i: int, epoch: int, seed: int, n: int = 8):
    """h0 .. h(n-1) of dataset index i."""
    h = lowbias32(((i & M32) * 0x9E3779B1 + (epoch & M32) * 0x85EBCA77 + (seed & M32) * 0xC2B2AE3D) & M32)
    out = [h]
    for _ in range(n - 1):
        h = lowbias32((h + GOLD) & M32)
        out.append(h)
    return out


def crop_one(i, epoch, seed, pad, flip_enabled):
    h = chain(i, epoch, seed, 3)
    span = 2 * pad + 1
    return (h[0] * span) >> 32, (h[1] * span) >> 32, (h[2] >> 31) if flip_enabled else 0


def clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def box_one(i, epoch, seed, H, W, prob):
    """(apply, y1, y2, x1, x2, area) of dataset index i; area is 0 when not applied."""
    h = chain(i, epoch, seed, 8)
    apply = h[3] < int(prob * 4294967296.0)
    side = max((h[4] * H) >> 32, (h[5] * H) >> 32)
    cy, cx = (h[6] * H) >> 32, (h[7] * W) >> 32
    half = side // 2
    y1, y2 = clip(cy - half, 0, H), clip(cy + half, 0, H)
    x1, x2 = clip(cx - half, 0, W), clip(cx + half, 0, W)
    return apply, y1, y2, x1, x2, ((y2 - y1) * (x2 - x1) if apply else 0)


def boxes(idx, epoch, seed, H, W, prob):
    """Arrays (apply bool, y1, y2, x1, x2 int64, wb float32) for the dataset indices idx."""
    rows = [box_one(int(i), epoch, seed, H, W, prob) for i in idx]
    a = np.array([r[0] for r in rows], dtype=bool)
    g = np.array([r[1:5] for r in rows], dtype=np.int64).reshape(-1, 4)
    area = np.array([r[5] for r in rows], dtype=np.float32)
    return a, g[:, 0], g[:, 1], g[:, 2], g[:, 3], area / np.float32(H * W)


def f32_bits(v) -> int:
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def bits_f32(b: int) -> np.float32:
    return np.float32(struct.unpack("<f", struct.pack("<I", b & M32))[0])


def pack(a, b, wb) -> np.ndarray:
    """int64 mixed labels: a | b << 8 | float32_bits(wb) << 32 (numpy twin of loss.pack_mixed)."""
    a, b, wb = np.broadcast_arrays(np.asarray(a), np.asarray(b), np.asarray(wb, dtype=np.float32))
    out = [(int(x) | (int(y) << 8) | (f32_bits(w) << 32)) for x, y, w in zip(a.ravel(), b.ravel(), wb.ravel())]
    return np.array([v - (1 << 64) if v >= (1 << 63) else v for v in out], dtype=np.int64).reshape(a.shape)


def unpack(y):
    """(a, b, wb float32) of int64 mixed labels (numpy twin of loss.unpack_mixed)."""
    y = np.asarray(y, dtype=np.int64)
    u = [int(v) & 0xFFFFFFFFFFFFFFFF for v in y.ravel()]
    a = np.array([v & 0xFF for v in u], dtype=np.int64).reshape(y.shape)
    b = np.array([(v >> 8) & 0xFF for v in u], dtype=np.int64).reshape(y.shape)
    wb = np.array([bits_f32(v >> 32) for v in u], dtype=np.float32).reshape(y.shape)
    return a, b, wb


def source_pixel(img, c, yo, xo, dy, dx, flip, pad):
    """The u8 value sample `img` [C,H,W] shows at output (c, yo, xo) under its draws."""
    _, H, W = img.shape
    xs = (W - 1 - xo if flip else xo) + dx - pad
    ys = yo + dy - pad
    return int(img[c, ys, xs]) if 0 <= xs < W and 0 <= ys < H else 0


def mixed_u8(images, idx, idx2, pad, flip_enabled, seed, epoch, prob):
    """The u8 batch [B,C,H,W] before ToTensor, pixel by pixel, and the per-position (apply, box, area)."""
    if images.ndim == 3:
        images = images[:, None]
    _, C, H, W = images.shape
    out = np.zeros((len(idx), C, H, W), dtype=np.uint8)
    info = []
    for s, (i, i2) in enumerate(zip(idx, idx2)):
        i, i2 = int(i), int(i2)
        da, db = crop_one(i, epoch, seed, pad, flip_enabled), crop_one(i2, epoch, seed, pad, flip_enabled)
        apply, y1, y2, x1, x2, area = box_one(i, epoch, seed, H, W, prob)
        info.append((apply, y1, y2, x1, x2, area))
        for yo in range(H):
            for xo in range(W):
                inside = apply and y1 <= yo < y2 and x1 <= xo < x2
                src, d = (images[i2], db) if inside else (images[i], da)
                for c in range(C):
                    out[s, c, yo, xo] = source_pixel(src, c, yo, xo, d[0], d[1], d[2], pad)
    return out, info


def batch(images, labels, idx, idx2, mean, std, pad=0, flip=False, seed=0, epoch=0, prob=1.0):
    """(x f32 [B,C,H,W], y i64 [B] mixed labels) of slk_image_batch_mix."""
    if images.ndim == 3:
        images = images[:, None]
    _, C, H, W = images.shape
    u8, info = mixed_u8(images, idx, idx2, pad, flip, seed, epoch, prob)
    m = np.asarray(mean, dtype=np.float32).reshape(-1, 1, 1)
    sd = np.asarray(std, dtype=np.float32).reshape(-1, 1, 1)
    x = ((u8.astype(np.float32) / np.float32(255) - m) / sd).astype(np.float32)
    y = np.zeros(len(idx), dtype=np.int64)
    for s, (i, i2) in enumerate(zip(idx, idx2)):
        area = info[s][5]
        a, b = int(labels[int(i)]), int(labels[int(i2)])
        y[s] = pack(a, b, np.float32(area) / np.float32(H * W)) if area > 0 else a
    return x, y


def synthetic(n, shape, seed):
    """A u8 dataset [n, *shape] with no two neighbouring pixels alike, and labels in [0, 10)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(n,) + tuple(shape), dtype=np.uint8), rng.integers(0, 10, size=n).astype(np.uint8)
