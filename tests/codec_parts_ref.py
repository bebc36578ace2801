"""Test infrastructure: the lossless cut codec's stream (the contract at the top of tests/test_codec_gpu.py), its split
into the independent parts of a server chunk and the addressing of the fused consumers, restated in plain numpy; the
mask families of tests/test_codec_parts_gpu.py; and the comparisons that test uses. tests/test_codec_parts_ref_cpu.py
pins all of it without a GPU.

The stream of a flat bool vector set_ of n elements (blocks of 2048 elements, words of 32):
  mask_words  bit i % 32 of word i / 32 = set_[i]               (little-endian within a word, unused high bits 0)
  counts[k]   set elements of block k,  offsets = exclusive scan of counts,  total = their sum
  ranks[w]    set elements before word w = the vals index of word w's first set element
  pack        values[set_] in element order
A chunk [B, 32, 26, 26] of part_b samples a part is B / part_b such streams, each with its own element 0: sample b
belongs to part b // part_b and is sample b - part_b (b // part_b) of it. A sample is 21,632 elements = 676 words, so
a part always starts on a word.

The fused consumers (csrc/slk_x3.hip: cut_unpack_x3_kernel, conv2_dgrad_x3_kernel's PACK path) find an element through
a device table with one row of pointers per part, in the column orders of include/slk.h that OFFSETS_COLS, UNPACK_COLS
and PACK_COLS repeat. `model_pack_parts` / `model_unpack_parts` restate that addressing over a dictionary of arrays:
element e of sample b sits in word w = 676 lb + e / 32 of its part, and where bit e % 32 of mask[w] is set its value is
vals[ranks[w] + popcount(mask[w] below that bit)]. Their `wrong` argument selects one of three mistakes
(WRONG_VARIANTS) that the comparisons below must notice; a store outside its array is dropped, as a model must.

Mask families, each a function of (B, seed) returning a bool tensor [B, 32, 26, 26]:
  random       ReLU of a standard normal: the distribution of the zero pattern of `cut` in
               test_x3_lo_exact_gpu.dgrad_case (the GPU tests that build a dgrad_case use its own cut's pattern)
  degenerate   sample s takes pattern s % 8 of DEGENERATE: nothing, everything, element 0, element 21,631, pixel 675
               of every channel, the elements = 31 mod 32 (bit 31 of every word), = 0 mod 32 (bit 0), 0x55555555 words
  sparse       density 1/64
  empty_part(part_b)   random with every sample of part 1 cleared (unchanged where there is no part 1)
"""
import numpy as np
import torch

A_SAMPLE = 32 * 26 * 26          # 21,632 elements of one cut sample
A_WORDS = A_SAMPLE // 32         # 676 mask words
A_PIX = 26 * 26
CB = 2048                        # elements of a codec block
SHAPE = (32, 26, 26)

OFFSETS_COLS = ("mask", "counts", "offsets", "total", "ranks")    # slk_cut_offsets_ranks_parts
UNPACK_COLS = ("vals", "mask", "ranks")                            # slk_cut_unpack_x3_parts
PACK_COLS = ("mask", "ranks", "vals")                              # slk_conv2_dgrad_x3_pack_parts

WRONG_VARIANTS = ("rank_counts_own_bit", "part_is_b_mod_part_b", "columns_exchanged")


# ----------------------------------------------------------------------------- the stream
def _flat(set_):
    return np.ascontiguousarray(np.asarray(set_, dtype=bool)).reshape(-1)


def _padded(a, m):
    out = np.zeros((a.size + m - 1) // m * m, dtype=a.dtype)
    out[:a.size] = a
    return out


def mask_words(set_):
    return np.packbits(_padded(_flat(set_), 32), bitorder="little").view("<u4").astype(np.uint32)


def set_of_words(words, n):
    """The inverse of mask_words: bool [n]."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def _word_counts(set_):
    return _padded(_flat(set_), 32).reshape(-1, 32).sum(1, dtype=np.int64)


def counts(set_):
    return _padded(_flat(set_), CB).reshape(-1, CB).sum(1, dtype=np.int64)


def offsets(set_):
    c = counts(set_)
    return np.cumsum(c) - c


def total(set_):
    return int(_flat(set_).sum())


def ranks(set_):
    c = _word_counts(set_)
    return np.cumsum(c) - c


def pack(values, set_):
    return np.asarray(values).reshape(-1)[_flat(set_)]


def stream(set_):
    """Every array of one stream: {"mask", "counts", "offsets", "total", "ranks"} (int64 but the uint32 mask)."""
    return {"mask": mask_words(set_), "counts": counts(set_), "offsets": offsets(set_),
            "total": np.array([total(set_)], dtype=np.int64), "ranks": ranks(set_)}


# ----------------------------------------------------------------------------- parts
def part_index(b, part_b):
    return b // part_b


def check_part_b(B, part_b):
    if part_b <= 0 or B % part_b:
        raise ValueError(f"part_b {part_b} must divide the chunk's {B} samples")
    return B // part_b


def split_parts(t, part_b):
    """t [B, ...] (numpy or torch) -> the B / part_b parts [part_b, ...], in part order."""
    B = t.shape[0]
    idx = part_index(np.arange(B), part_b)
    return [t[np.flatnonzero(idx == k)] for k in range(check_part_b(B, part_b))]


def pack_parts(values, set_, part_b):
    """What each part's values buffer holds after the packed dgrad: values at the part's own set positions."""
    v = np.asarray(values)
    s = np.asarray(set_, dtype=bool)
    return [pack(vk, sk) for vk, sk in zip(split_parts(v, part_b), split_parts(s, part_b))]


def table_rows(cols, nparts, vals="vals"):
    """The device table as the tests write it: row k names part k's arrays in the entry's column order (`vals`: the
    name of the array its vals column points to, "gvals" for the gradient direction)."""
    return [tuple((k, vals if c == "vals" else c) for c in cols) for k in range(nparts)]


# ----------------------------------------------------------------------------- the consumers' addressing
def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8)).reshape(-1, 32).sum(1, dtype=np.int64)


def _columns(mem, row, want, wrong):
    """The arrays a kernel takes for the column names `want` from a table row written in that order; the
    columns_exchanged mistake reads the row in the other consumer's order."""
    order = want
    if wrong == "columns_exchanged":
        order = UNPACK_COLS if want == PACK_COLS else PACK_COLS
    got = {name: mem[row[i]] for i, name in enumerate(order)}
    return got["mask"].view(np.uint32), got["ranks"].view(np.int32), got["vals"].view(np.uint32)


def _locate(B, part_b, wrong):
    for b in range(B):
        if wrong == "part_is_b_mod_part_b":
            yield b, b % part_b, b // part_b
        else:
            part = b // part_b
            yield b, part, b - part * part_b


def _addresses(mk, rk, lb, wrong):
    """(set flags, vals index) of the 21,632 elements of the part's sample lb; words outside the mask read as 0."""
    e = np.arange(A_SAMPLE)
    w, bit = lb * A_WORDS + (e >> 5), (e & 31).astype(np.uint64)
    ok = (w >= 0) & (w < min(mk.size, rk.size))
    wc = np.where(ok, w, 0)
    m = np.where(ok, mk[wc], 0).astype(np.uint64)
    below = m & ((np.uint64(1) << bit) - np.uint64(1))
    if wrong == "rank_counts_own_bit":
        below = m & ((np.uint64(2) << bit) - np.uint64(1))
    r = rk[wc].astype(np.int64) + _popcount(below.astype(np.uint32))
    return ((m >> bit) & np.uint64(1)).astype(bool), r


def model_pack_parts(values, mem, table, part_b, wrong=None):
    """The packed dgrad's stores: values [B, 21632] f32 written into the vals arrays the table names. mem maps a
    table cell to its array (uint32 / int32 / float32, changed in place)."""
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, A_SAMPLE)
    for b, part, lb in _locate(values.shape[0], part_b, wrong):
        if not 0 <= part < len(table):
            continue
        mk, rk, vl = _columns(mem, table[part], PACK_COLS, wrong)
        on, r = _addresses(mk, rk, lb, wrong)
        on &= (r >= 0) & (r < vl.size)
        vl[r[on]] = values[b].view(np.uint32)[on]


def model_unpack_parts(B, mem, table, part_b, wrong=None):
    """The unpack's gathers: the dense f32 chunk [B, 21632] (+0 where unset, NaN for a read outside an array)."""
    out = np.zeros((B, A_SAMPLE), dtype=np.float32)
    for b, part, lb in _locate(B, part_b, wrong):
        if not 0 <= part < len(table):
            out[b] = np.nan
            continue
        mk, rk, vl = _columns(mem, table[part], UNPACK_COLS, wrong)
        on, r = _addresses(mk, rk, lb, wrong)
        inside = (r >= 0) & (r < vl.size)
        padded = np.append(vl, np.float32(np.nan).view(np.uint32))
        out[b] = np.where(on, padded[np.where(inside, r, vl.size)].view(np.float32), np.float32(0))
    return out


def part_memory(values, set_, part_b, front=1):
    """The arrays of every part for the models: its stream, its packed `values` (f32 [B, ...]; unpack's input) and a
    NaN-filled gradient buffer of front + n + 1 floats. Returns (mem, gradient buffers, totals)."""
    mem, grads, tots = {}, [], []
    v = np.ascontiguousarray(values, dtype=np.float32)
    for k, (vk, sk) in enumerate(zip(split_parts(v, part_b), split_parts(np.asarray(set_, dtype=bool), part_b))):
        st = stream(sk)
        buf = np.full(front + sk.size + 1, np.nan, dtype=np.float32)
        mem[k, "mask"], mem[k, "ranks"] = st["mask"], st["ranks"].astype(np.int32)
        mem[k, "vals"], mem[k, "gvals"] = pack(vk, sk).astype(np.float32), buf[front:]
        grads.append(buf)
        tots.append(int(st["total"][0]))
    return mem, grads, tots


# ----------------------------------------------------------------------------- comparisons (used on the GPU)
def assert_stream(got, set_, what=""):
    """got: {"mask", "counts", "offsets", "total", "ranks"} integer arrays == the stream of set_."""
    want = stream(set_)
    for name in OFFSETS_COLS:
        g = np.asarray(got[name]).reshape(-1)
        g = g.astype(np.int64) & 0xFFFFFFFF if name == "mask" else g.astype(np.int64)       # int32 words: their bits
        bad = g.shape != want[name].shape or not np.array_equal(g, want[name].astype(np.int64))
        assert not bad, f"{what}: {name} differs from the numpy stream"


def assert_packed(buf, base, want, what=""):
    """buf (f32, a NaN-filled allocation whose values start at `base`): buf[base : base + t] == want as float64,
    and every float in front of the base and from base + t on is still NaN."""
    buf = np.asarray(buf, dtype=np.float32).reshape(-1)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    t = want.size
    bad = buf[base:base + t].astype(np.float64) != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {t} packed values differ (first at {int(np.argmax(bad))})"
    assert np.isnan(buf[:base]).all(), f"{what}: a float in front of the base was written"
    assert np.isnan(buf[base + t:]).all(), f"{what}: written at or beyond the total {t}"


def assert_packed_parts(bufs, bases, values, set_, part_b, what=""):
    """Every part's allocation against the float64 `values` [B, ...] at the part's own set positions."""
    want = pack_parts(np.asarray(values, dtype=np.float64), set_, part_b)
    assert len(bufs) == len(want)
    for k, (buf, base, w) in enumerate(zip(bufs, bases, want)):
        assert_packed(buf, base, w, f"{what} part {k}")
    return want


def assert_unpacked(dense, values, set_, what=""):
    """dense f32 [B, ...] == values where set, +0 elsewhere, bit for bit."""
    want = np.where(np.asarray(set_, dtype=bool), np.asarray(values, dtype=np.float32), np.float32(0))
    got = np.asarray(dense, dtype=np.float32).reshape(want.shape)
    bad = got.view(np.uint32) != want.astype(np.float32).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} unpacked elements differ"


# ----------------------------------------------------------------------------- mask families
def random(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B,) + SHAPE, generator=g).clamp_min(0.0) != 0


def _degenerate_pattern(j):
    e = torch.arange(A_SAMPLE)
    if j == 0:
        return torch.zeros(A_SAMPLE, dtype=torch.bool)
    if j == 1:
        return torch.ones(A_SAMPLE, dtype=torch.bool)
    if j == 2:
        return e == 0
    if j == 3:
        return e == A_SAMPLE - 1
    if j == 4:
        return e % A_PIX == A_PIX - 1
    if j == 5:
        return e % 32 == 31
    if j == 6:
        return e % 32 == 0
    return e % 2 == 0                                                   # 0x55555555 words


DEGENERATE = ("none", "all", "element 0", "element 21631", "pixel 675", "bit 31", "bit 0", "0x55555555")


def degenerate(B, seed=0):
    pats = torch.stack([_degenerate_pattern(j) for j in range(8)])
    return pats[torch.arange(B) % 8].reshape((B,) + SHAPE).clone()


def sparse(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B,) + SHAPE, generator=g) < 1.0 / 64


def clear_part(set_, part_b, part=1):
    """set_ with every sample of `part` cleared (unchanged where the chunk has no such part)."""
    out = set_.clone()
    if part < out.shape[0] // part_b:
        out[part * part_b:(part + 1) * part_b] = False
    return out


def empty_part(part_b):
    return lambda B, seed: clear_part(random(B, seed), part_b)


FAMILIES = ("random", "degenerate", "sparse", "empty_part")


def family(name, B, seed, part_b=None):
    if name == "empty_part":
        return empty_part(part_b)(B, seed)
    return {"random": random, "degenerate": degenerate, "sparse": sparse}[name](B, seed)


# ----------------------------------------------------------------------------- a per-element loop (the pin)
def loop_parts(values, set_, part_b):
    """Every part's stream and packed values by one Python loop over the elements, written without the functions
    above: [{"mask", "counts", "offsets", "total", "ranks", "vals"}] as Python lists."""
    B = len(set_)
    assert B % part_b == 0
    v = np.asarray(values).reshape(B, -1)
    s = np.asarray(set_, dtype=bool).reshape(B, -1)
    out = []
    for k in range(B // part_b):
        p = {name: [] for name in OFFSETS_COLS + ("vals",)}
        seen, word, in_block = 0, 0, 0
        n = part_b * A_SAMPLE
        for i in range(n):
            b, e = k * part_b + i // A_SAMPLE, i % A_SAMPLE
            if i % CB == 0:
                p["offsets"].append(seen)
                in_block = 0
            if i % 32 == 0:
                p["ranks"].append(seen)
                word = 0
            if s[b, e]:
                word |= 1 << (i % 32)
                p["vals"].append(v[b, e])
                seen += 1
                in_block += 1
            if i % 32 == 31 or i == n - 1:
                p["mask"].append(word)
            if i % CB == CB - 1 or i == n - 1:
                p["counts"].append(in_block)
        p["total"] = [seen]
        out.append(p)
    return out
