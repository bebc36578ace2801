"""GPU: the fused kernels of the lossless cut codec alone, against float64 and the numpy stream of
tests/codec_parts_ref.py: slk_conv2_dgrad_x3_pack where its LDS double buffer is reused, and the three multi-part
entries slk_cut_offsets_ranks_parts, slk_cut_unpack_x3_parts and slk_conv2_dgrad_x3_pack_parts.

Why these sizes. A workgroup of the packed dgrad walks per = ceil(3 B / 256) pairs and receives pair pr + 1's mask words
and word ranks by LDS-DMA into buffer (q + 1) & 1 while pair pr computes; a buffer an epilogue has read is overwritten
by a prefetch that is consumed only from per = 3. B = 171 is the smallest batch with per = 3 (a workgroup is exactly
one sample) and B = 258 has per = 4 (sample and part boundaries fall inside a workgroup's range); the other exact
tests stop at per = 2. Operands are the exact classes dp14 and both of test_x3_lo_exact_gpu.dgrad_case, so every packed
value must EQUAL the three-term float64 expectation (as float64: the sign of a zero sum is not compared), at a tight and
a loose scale bound.

Masks come from four families (codec_parts_ref: random = the zero pattern of the case's own cut, degenerate, sparse,
empty_part): samples with no set element, every element, only element 0 or 21,631, only the last pixel of every
channel, only bit 31 or bit 0 of every word - the edges of ranks[w] + popc(m & ((1 << bit) - 1)) and of the 10-word
window a pair stages. Every mask and rank array the kernels read is first compared with the numpy stream.

Parts. Each part is encoded on its own into separately allocated buffers, made in a shuffled order so that the table,
not the memory order, says which buffers a sample uses. Part k's gradient values start 4 + k % 4 floats into a NaN-filled
allocation (the base is 4-byte aligned only, k % 4 floats past a 16-byte boundary, and there is always a float in front
of it to look at); the unpack's values start k % 4 floats into theirs. Checked: each part against float64 at its own
set positions, NaN beyond its total and in front of its base, the concatenation bitwise equal to the single-part
entry, an all-clear part's buffer untouched; the images of the multi-part unpack bit for bit the numpy split and the
whole-batch unpack; counts / offsets / total / ranks of every part with a guard element behind each; and, under a
captured graph, that swapping table rows on the device between replays moves the outputs (dist.Hub._part_tables
writes its tables once and relies on the kernels reading them at run time).

Every comparison is exact: bits, or NaN-ness of guards."""
import numpy as np
import pytest
import torch

import codec_parts_ref as R
from test_x3_lo_exact_gpu import _amax_forms, _check_images, _nan, _real_act, dgrad_case

pytestmark = pytest.mark.gpu

PART_BS = {5: (1, 5), 171: (1, 3, 19, 57, 171), 258: (1, 2, 43, 129)}
DEPTH = [(171, 3), (258, 4)]                     # (B, per)
FRONT = 4                                        # floats in front of a part's gradient values, before the k % 4


@pytest.fixture(scope="module")
def cases(gpu):
    """dgrad_case(cls, B) made once per module: (dpooled, W2, code, cut, float64 expectation on the host)."""
    made = {}

    def get(cls, B):
        if (cls, B) not in made:
            dp, W2, code, _, _, cut, g64, _ = dgrad_case(cls, B, 3100 + B, gpu)
            made[cls, B] = (dp, W2, code, cut, g64.cpu().numpy())
        return made[cls, B]
    yield get
    made.clear()


def _set_of(fam, B, cut, part_b):
    own = (cut != 0).cpu()
    if fam == "random":
        return own
    if fam == "empty_part":
        return R.clear_part(own, part_b)
    return R.family(fam, B, 3000 + B)


def _source(set_, cut):
    """A tensor with the zero pattern set_: the cut's own values where it has them, 1 elsewhere."""
    s = set_.to(cut.device)
    return torch.where(s, torch.where(cut != 0, cut, torch.ones_like(cut)), torch.zeros_like(cut)).contiguous()


def _host(t):
    return t.cpu().numpy()


def _encode(codec, key, x):
    n = x.numel()
    bk = codec.buffers(key, n, x.device)
    codec.encode(x, bk)
    return bk, codec.ranks(key, n, bk)


def _check_stream(bk, rk, set_np, what):
    R.assert_stream({"mask": _host(bk[0]), "counts": _host(bk[1]), "offsets": _host(bk[2]), "total": _host(bk[3]),
                     "ranks": _host(rk)}, set_np, what)


def _table(rows, cols, dev):
    """int64 device table: one row per part, the cells' addresses in the entry's column order."""
    return torch.tensor([[row[c].data_ptr() for c in cols] for row in rows], dtype=torch.int64).to(dev)


def _layout(codec, src, set_np, part_b, seed):
    """Every part of src encoded on its own, in a shuffled order of allocation: [{"mask", "ranks", "cvals" (the packed
    cut), "total", "alloc" / "base" / "vals" (the NaN-filled gradient buffer)}] in part order."""
    B, dev = src.shape[0], src.device
    n = part_b * R.A_SAMPLE
    parts = [None] * (B // part_b)
    order = np.random.default_rng(seed).permutation(len(parts)).tolist()
    if order == sorted(order):
        order.reverse()
    for k in order:
        bk, rk = _encode(codec, ("part", part_b, k), src[k * part_b:(k + 1) * part_b])
        alloc = _nan((FRONT + 3 + n + 2,), dev)
        base = FRONT + k % 4
        parts[k] = {"bk": bk, "mask": bk[0], "ranks": rk, "cvals": bk[4], "alloc": alloc, "base": base,
                    "vals": alloc[base:base + n]}
    for k, (p, sk) in enumerate(zip(parts, R.split_parts(set_np, part_b))):
        assert p["vals"].data_ptr() % 16 == 4 * (k % 4)
        p["total"] = R.total(sk)
        _check_stream(p["bk"], p["ranks"], sk, f"part {k} of {part_b} samples")
    return parts


def _per(B):
    return -(-3 * B // 256)


# ----------------------------------------------------------------------------- slk_conv2_dgrad_x3_pack at depth
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("cls", ["dp14", "both"])
@pytest.mark.parametrize("B,per", DEPTH)
def test_packed_dgrad_at_depth(gpu, cases, B, per, cls, fam):
    """The single-part entry where a workgroup walks 3 and 4 pairs: vals[:t] == the float64 expectation at the set
    positions, NaN from t on and in front of the base."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    assert _per(B) == per
    dp, W2, code, cut, g64 = cases(cls, B)
    set_ = _set_of(fam, B, cut, PART_BS[B][2])
    set_np = set_.numpy()
    bk, rk = _encode(CutCodec(), "whole", _source(set_, cut))
    _check_stream(bk, rk, set_np, f"{fam} B = {B}")
    n = cut.numel()
    want = R.pack(g64, set_np)
    assert int(bk[3].item()) == want.size and 0 < want.size < n
    for name, dpa in _amax_forms(dp):
        buf = _nan((n + 2,), gpu)
        ops.conv2_dgrad_x3_pack(dp, code, W2, dpa, bk[0], rk, buf[1:n + 1])
        R.assert_packed(_host(buf), 1, want, f"packed dgrad {cls} {fam} B = {B} ({name})")


@pytest.mark.parametrize("B,per", DEPTH)
def test_packed_dgrad_of_an_all_clear_mask_writes_nothing(gpu, cases, B, per):
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    dp, W2, code, cut, _ = cases("dp14", B)
    bk, rk = _encode(CutCodec(), "clear", torch.zeros_like(cut))
    assert int(bk[3].item()) == 0 and not bk[0].any() and not rk.any()
    n = cut.numel()
    for name, dpa in _amax_forms(dp):
        buf = _nan((n + 2,), gpu)
        ops.conv2_dgrad_x3_pack(dp, code, W2, dpa, bk[0], rk, buf[1:n + 1])
        assert torch.isnan(buf).all(), name


# ----------------------------------------------------------------------------- slk_conv2_dgrad_x3_pack_parts
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("cls", ["dp14", "both"])
@pytest.mark.parametrize("B,per", DEPTH)
def test_packed_dgrad_parts(gpu, cases, B, per, cls, fam):
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    dp, W2, code, cut, g64 = cases(cls, B)
    n = cut.numel()
    codec = CutCodec()
    forms = _amax_forms(dp)
    whole = {}                                   # the single-part entry's output per mask: {form: bits of vals[:t]}
    for part_b in PART_BS[B]:
        nparts = B // part_b
        if fam == "empty_part" and nparts < 2:
            continue                             # no part 1 to clear: the random family's case
        set_ = _set_of(fam, B, cut, part_b)
        set_np = set_.numpy()
        src = _source(set_, cut)
        key = part_b if fam == "empty_part" else 0
        if key not in whole:
            bk, rk = _encode(codec, ("whole", key), src)
            t = int(bk[3].item())
            whole[key] = {}
            for name, dpa in forms:
                one = _nan((n,), gpu)
                ops.conv2_dgrad_x3_pack(dp, code, W2, dpa, bk[0], rk, one)
                whole[key][name] = _host(one)[:t].view(np.uint32)
        parts = _layout(codec, src, set_np, part_b, 31 * B + part_b)
        table = _table([{"mask": p["mask"], "ranks": p["ranks"], "vals": p["vals"]} for p in parts], R.PACK_COLS, gpu)
        for name, dpa in forms:
            what = f"packed dgrad parts {cls} {fam} B = {B} part_b = {part_b} ({name})"
            for p in parts:
                p["alloc"].fill_(float("nan"))
            ops.conv2_dgrad_x3_pack_parts(dp, code, W2, dpa, table, part_b)
            bufs = [_host(p["alloc"]) for p in parts]
            bases = [p["base"] for p in parts]
            want = R.assert_packed_parts(bufs, bases, g64, set_np, part_b, what)
            assert [w.size for w in want] == [p["total"] for p in parts]
            cat = np.concatenate([b[s:s + w.size] for b, s, w in zip(bufs, bases, want)]).view(np.uint32)
            assert np.array_equal(cat, whole[key][name]), f"{what}: the parts' concatenation != the single-part entry"
            if fam == "empty_part":
                assert parts[1]["total"] == 0 and np.isnan(bufs[1]).all(), f"{what}: the all-clear part was written"


def test_packed_dgrad_parts_refuses_a_part_b_that_does_not_divide(gpu, cases):
    from splitcnn import ops
    dp, W2, code, _, _ = cases("dp14", 171)
    dpa = ops.row_amax(dp)
    table = torch.zeros((171, 3), dtype=torch.int64, device=gpu)
    for part_b in (0, 2, 172, -57):
        with pytest.raises(ValueError, match="must divide"):
            ops.conv2_dgrad_x3_pack_parts(dp, code, W2, dpa, table, part_b)


# ----------------------------------------------------------------------------- slk_cut_unpack_x3_parts
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("B", [5, 171])
def test_unpack_parts_into_images(gpu, B, fam):
    """Real-valued cuts with each family's pattern forced onto them: the multi-part unpack's images == the numpy
    split == the whole-batch unpack's images, from value buffers that start k % 4 floats into a NaN-filled allocation."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    act = _real_act(B, 3400 + B)
    tiny = float(np.finfo(np.float32).tiny)
    codec = CutCodec()
    done = {}
    for part_b in PART_BS[B]:
        nparts = B // part_b
        if fam == "empty_part" and nparts < 2:
            continue
        set_ = R.family(fam, B, 3500 + B, part_b)
        forced = torch.where(set_, act.abs() + tiny, torch.zeros_like(act)).contiguous()
        assert torch.equal(forced != 0, set_)
        forced = forced.to(gpu)
        amx = ops.row_amax(forced)
        key = part_b if fam == "empty_part" else 0
        if key not in done:
            bk, rk = _encode(codec, ("whole", key), forced)
            _check_stream(bk, rk, set_.numpy(), f"{fam} B = {B}")
            img = torch.full((ops.conv2_act16_bytes(B),), 0xA5, dtype=torch.uint8, device=gpu)
            ops.cut_unpack_x3(bk[4], bk[0], rk, amx, img)
            _check_images(img, B, forced, amx, f"cut_unpack_x3 {fam} B = {B}")
            done[key] = img
        parts = _layout(codec, forced, set_.numpy(), part_b, 37 * B + part_b)
        rows = []
        for k, p in enumerate(parts):
            t = p["total"]
            alloc = _nan((k % 4 + t + 1,), gpu)
            alloc[k % 4:k % 4 + t].copy_(p["cvals"][:t])
            rows.append({"vals": alloc[k % 4:], "mask": p["mask"], "ranks": p["ranks"]})
            assert rows[-1]["vals"].data_ptr() % 16 == 4 * (k % 4)
        table = _table(rows, R.UNPACK_COLS, gpu)
        img = torch.full_like(done[key], 0xA5)
        ops.cut_unpack_x3_parts(table, part_b, amx, img)
        what = f"cut_unpack_x3_parts {fam} B = {B} part_b = {part_b}"
        _check_images(img, B, forced, amx, what)
        assert torch.equal(img, done[key]), f"{what}: differs from the whole-batch unpack"


# ----------------------------------------------------------------------------- slk_cut_offsets_ranks_parts
def _mask_parts(nparts, n, seed):
    """Random words with the bits past n cleared; with three or more parts, part 1 all clear and part 2 all set."""
    rng = np.random.default_rng(seed)
    nw = (n + 31) // 32
    words = rng.integers(0, 2 ** 32, (nparts, nw), dtype=np.uint64).astype(np.uint32)
    if nparts >= 3:
        words[1], words[2] = 0, 0xFFFFFFFF
    if n % 32:
        words[:, -1] &= np.uint32((1 << (n % 32)) - 1)
    return words


OFFSETS_CASES = [(p, n) for p in (1, 2, 7) for n in (1, 33, 2049, 65_541)] + \
                [(2, 2048 * 1100 + 7), (2, 2048 * 12_289 + 5)]


@pytest.mark.parametrize("nparts,n", OFFSETS_CASES)
def test_offsets_ranks_parts(gpu, nparts, n):
    """counts, offsets, total and ranks of every part == the numpy stream and == CutCodec.offsets + CutCodec.ranks
    run part by part; the guard element behind each array keeps its -1. n = 2048 * 1100 + 7 has more blocks than
    the scan has threads, 2048 * 12,289 + 5 more than it stages in LDS."""
    from splitcnn import _lib, ops
    from splitcnn.codec import CutCodec
    words = _mask_parts(nparts, n, 41 * nparts + n)
    nw, nb = words.shape[1], _lib.query("slk_cut_blocks", n)
    assert nb == (n + R.CB - 1) // R.CB
    sizes = {"counts": nb, "offsets": nb, "total": 1, "ranks": nw}
    rows = []
    for k in range(nparts):
        row = {"mask": torch.from_numpy(words[k].view(np.int32)).to(gpu)}
        for name, size in sizes.items():
            row[name] = torch.full((size + 1,), -1, dtype=torch.int32, device=gpu)
        rows.append(row)
    ops.cut_offsets_ranks_parts(_table(rows, R.OFFSETS_COLS, gpu), n)
    codec = CutCodec()
    for k, row in enumerate(rows):
        what = f"part {k} of {nparts}, n = {n}"
        set_ = R.set_of_words(words[k], n)
        assert nparts < 3 or k not in (1, 2) or int(set_.sum()) == (0 if k == 1 else n)
        R.assert_stream({name: _host(t)[:-1] if name in sizes else _host(t) for name, t in row.items()}, set_, what)
        for name in sizes:
            assert int(row[name][-1].item()) == -1, f"{what}: the guard behind {name} was written"
        bk = codec.buffers(("one", k), n, gpu)
        bk[0].copy_(row["mask"])
        codec.offsets(n, bk)
        rk = codec.ranks(("one", k), n, bk)
        for name, t in (("counts", bk[1]), ("offsets", bk[2]), ("total", bk[3]), ("ranks", rk)):
            assert torch.equal(row[name][:-1], t), f"{what}: {name} != the single-part codec's"


# ----------------------------------------------------------------------------- the tables are device memory
def test_replay_follows_the_tables(gpu, cases):
    """The offsets / ranks launches and the packed dgrad captured in one graph at B = 171, part_b = 57. A replay
    recomputes every part; after rows 0 and 2 of both tables are exchanged by device copies on the stream, the next
    replay packs samples 0-56 at part 2's mask into part 2's buffer and samples 114-170 into part 0's."""
    from splitcnn import ops
    from splitcnn.codec import CutCodec
    from splitcnn.graphs import capture
    B, part_b = 171, 57
    dp, W2, code, cut, g64 = cases("dp14", B)
    set_np = (cut != 0).cpu().numpy()
    n = part_b * R.A_SAMPLE
    parts = _layout(CutCodec(), cut, set_np, part_b, 53)
    t_off = _table([{"mask": p["bk"][0], "counts": p["bk"][1], "offsets": p["bk"][2], "total": p["bk"][3],
                     "ranks": p["ranks"]} for p in parts], R.OFFSETS_COLS, gpu)
    t_pack = _table([{"mask": p["mask"], "ranks": p["ranks"], "vals": p["vals"]} for p in parts], R.PACK_COLS, gpu)
    dpa = ops.row_amax(dp)

    def run():
        ops.cut_offsets_ranks_parts(t_off, n)
        ops.conv2_dgrad_x3_pack_parts(dp, code, W2, dpa, t_pack, part_b)

    graph, _ = capture(run, gpu)
    sets = R.split_parts(set_np, part_b)
    vals = R.split_parts(g64, part_b)

    def replay_and_check(perm, what):
        """perm[k] = the buffers sample group k uses."""
        for p in parts:
            p["alloc"].fill_(float("nan"))
            for t in (p["bk"][1], p["bk"][2], p["bk"][3], p["ranks"]):
                t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k, j in enumerate(perm):
            _check_stream(parts[j]["bk"], parts[j]["ranks"], sets[j], f"{what}: buffers {j}")
            R.assert_packed(_host(parts[j]["alloc"]), parts[j]["base"], R.pack(vals[k], sets[j]),
                            f"{what}: samples of part {k} into buffers {j}")

    replay_and_check((0, 1, 2), "replay")
    for t in (t_off, t_pack):
        row0 = t[0].clone()
        t[0].copy_(t[2])
        t[2].copy_(row0)
    replay_and_check((2, 1, 0), "replay after the row exchange")
    assert not np.array_equal(R.pack(vals[0], sets[2]), R.pack(vals[0], sets[0]))
