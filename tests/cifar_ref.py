"""TEST INFRASTRUCTURE: an independent numpy reference of the augmented batch slk_image_batch builds.

torchvision is not installed, so its semantics are restated here the slow, explicit way, sample by sample:
  RandomCrop(H, padding=pad): zero-pad the u8 image by `pad` on every side, cut the H x W window whose top left
                              corner is (dy, dx) in the padded image;
  RandomHorizontalFlip:       reverse the columns of the window if the sample's flip bit is set;
  ToTensor + Normalize:       (img.astype(f32) / f32(255) - mean) / std, all in float32 (oracle/mnist.py pins
                              that op sequence against torch for C = 1).
The draws are this file's own restatement of the documented hash (include/slk.h), in Python integers — nothing
here is imported from the package under test."""
import numpy as np

M32 = 0xFFFFFFFF


def lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def draws_one(i: int, epoch: int, seed: int, pad: int, flip: bool = True):
    e = ((i & M32) * 0x9E3779B1 + epoch * 0x85EBCA77 + seed * 0xC2B2AE3D) & M32
    h0 = lowbias32(e)
    h1 = lowbias32(h0 + 0x9E3779B9)
    h2 = lowbias32(h1 + 0x9E3779B9)
    span = 2 * pad + 1
    return (h0 * span) >> 32, (h1 * span) >> 32, (h2 >> 31) if flip else 0


def draws(idx, epoch: int, seed: int, pad: int, flip: bool = True):
    """(dy, dx, flip) int64 arrays for the dataset indices idx."""
    d = np.array([draws_one(int(i), epoch, seed, pad, flip) for i in idx], dtype=np.int64).reshape(-1, 3)
    return d[:, 0], d[:, 1], d[:, 2]


def normalize(img_u8: np.ndarray, mean, std) -> np.ndarray:
    """u8 [..., C, H, W] -> f32, ToTensor + Normalize per channel, every step in float32."""
    m = np.asarray(mean, dtype=np.float32).reshape(-1, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(-1, 1, 1)
    t = img_u8.astype(np.float32) / np.float32(255)
    return ((t - m) / s).astype(np.float32)


def crop_flip(img_u8: np.ndarray, dy: int, dx: int, flip: int, pad: int) -> np.ndarray:
    """One u8 image [C,H,W]: explicit zero padding, the window at (dy, dx), then the flip."""
    C, H, W = img_u8.shape
    padded = np.zeros((C, H + 2 * pad, W + 2 * pad), dtype=np.uint8)
    padded[:, pad:pad + H, pad:pad + W] = img_u8
    win = padded[:, dy:dy + H, dx:dx + W]
    return win[:, :, ::-1] if flip else win


def batch(images_u8, labels_u8, idx, mean, std, pad=0, flip=False, seed=0, epoch=0):
    """(x f32 [B,C,H,W], y i64 [B]) for the rows idx of images_u8 [N,C,H,W] ([N,H,W]: C = 1)."""
    if images_u8.ndim == 3:
        images_u8 = images_u8[:, None]
    idx = np.asarray(idx, dtype=np.int64)
    dy, dx, fl = draws(idx, epoch, seed, pad, flip)
    out = np.stack([crop_flip(images_u8[i], int(a), int(b), int(f), pad) for i, a, b, f in zip(idx, dy, dx, fl)]) \
        if len(idx) else np.zeros((0,) + images_u8.shape[1:], dtype=np.uint8)
    return normalize(out, mean, std), labels_u8[idx].astype(np.int64)
