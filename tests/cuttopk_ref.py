"""The top-k cut records of include/slk.h ("Top-k cut records") in plain numpy, over uint16 views of bf16 rows: a
stable sort of -mag, the record, decode and roundtrip. Test infrastructure: the kernels are held to this."""
import numpy as np
import torch

SAMPLE, HEAD, BITMAP, NAN, FMT_WORD = 16384, 16, 2048, 0x7FC0, 0x20
VALUES = HEAD + BITMAP


def record_bytes(k):
    return VALUES + 2 * k


def to_bits(t):
    """bf16 tensor -> uint16 numpy array of its bits."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)


def keep(bits, k):
    """bool [16384]: the first k of (mag descending, index ascending); None for a poisoned sample."""
    mag = (bits & 0x7FFF).astype(np.int32)
    if (mag >= 0x7F80).any():
        return None
    kept = np.zeros(SAMPLE, dtype=bool)
    kept[np.argsort(-mag, kind="stable")[:k]] = True
    return kept


def encode(x_bits, k):
    """uint16 [n, 16384] -> uint8 [n, 2064 + 2k]."""
    rec = np.zeros((len(x_bits), record_bytes(k)), dtype=np.uint8)
    for row, bits in zip(rec, x_bits):
        kept = keep(bits, k)
        row[:HEAD].view(np.uint32)[:] = (k, FMT_WORD, kept is None, 0)
        if kept is not None:
            row[HEAD:VALUES] = np.packbits(kept, bitorder="little")
            row[VALUES:].view(np.uint16)[:] = bits[kept]
    return rec


def decode(rec, k):
    """uint8 [n, 2064 + 2k] -> (uint16 [n, 16384], err_flag)."""
    out = np.full((len(rec), SAMPLE), NAN, dtype=np.uint16)
    flag = 0
    for row, o in zip(rec, out):
        w = row[:HEAD].view(np.uint32)
        kept = np.unpackbits(row[HEAD:VALUES], bitorder="little").astype(bool)
        if w[0] != k or w[1] != FMT_WORD or w[2] > 1 or w[3] != 0 or (w[2] == 0 and kept.sum() != k):
            flag = 1
        elif w[2] == 0:
            o[:] = 0
            o[kept] = row[VALUES:].view(np.uint16)
    return out, flag


def roundtrip(x_bits, k):
    out = np.full_like(x_bits, NAN)
    for bits, o in zip(x_bits, out):
        kept = keep(bits, k)
        if kept is not None:
            o[:] = np.where(kept, bits, 0)
    return out
