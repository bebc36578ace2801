"""CPU: tests/codec_parts_ref.py pinned without a GPU.

  * every mask family has the property its name states;
  * the numpy stream, the part split and the packed values equal a per-element Python loop (B = 3, part_b 1 and 3),
    and the table column orders equal the ones include/slk.h documents;
  * the model of the fused consumers' addressing reproduces the reference, and each of the three wrong variants
    (the rank counting the element's own bit, the part taken as b % part_b, the unpack and pack column orders
    exchanged) is refused by the comparisons tests/test_codec_parts_gpu.py applies to the kernels' outputs, on the
    degenerate family (B = 9, part_b = 3: all eight patterns, and b % 3 still names a part).
Putting any of the three mistakes into the reference itself (ranks, part_index, the *_COLS tuples) fails the second
group."""
import os
import re

import numpy as np
import pytest
import torch

import codec_parts_ref as R
from conftest import ROOT


# ----------------------------------------------------------------------------- families
def test_random_family_is_a_relu_pattern():
    s = R.random(4, 7)
    assert s.dtype == torch.bool and tuple(s.shape) == (4, 32, 26, 26)
    g = torch.Generator().manual_seed(7)
    assert torch.equal(s, torch.randn((4, 32, 26, 26), generator=g) > 0)
    assert 0.49 < float(s.float().mean()) < 0.51
    assert torch.equal(s, R.random(4, 7)) and not torch.equal(s, R.random(4, 8))


def test_degenerate_family_patterns():
    B = 17
    s = R.degenerate(B).reshape(B, -1).numpy()
    assert len(R.DEGENERATE) == 8
    for b in range(B):
        words = R.mask_words(s[b])
        on = np.flatnonzero(s[b])
        j = b % 8
        if j == 0:
            assert on.size == 0
        elif j == 1:
            assert on.size == R.A_SAMPLE and (words == 0xFFFFFFFF).all()
        elif j == 2:
            assert on.tolist() == [0] and words[0] == 1
        elif j == 3:
            assert on.tolist() == [21631] and words[-1] == 0x80000000 and not words[:-1].any()
        elif j == 4:
            assert on.tolist() == [676 * c + 675 for c in range(32)]
        elif j == 5:
            assert (words == 0x80000000).all()
        elif j == 6:
            assert (words == 1).all()
        else:
            assert (words == 0x55555555).all()
    assert np.array_equal(s[0], s[8]) and np.array_equal(s[3], s[11])


def test_sparse_family_density():
    s = R.sparse(6, 3)
    n = s.numel()                                             # a binomial count: mean n / 64, sigma sqrt(n / 64)
    assert abs(int(s.sum()) - n / 64) < 5 * (n / 64) ** 0.5
    assert s.reshape(6, -1).any(1).all()


@pytest.mark.parametrize("B,part_b", [(6, 2), (6, 1), (4, 4)])
def test_empty_part_family_clears_part_one(B, part_b):
    s, r = R.empty_part(part_b)(B, 5), R.random(B, 5)
    assert torch.equal(s, R.family("empty_part", B, 5, part_b))
    if B // part_b < 2:
        assert torch.equal(s, r)
        return
    lo, hi = part_b, 2 * part_b
    assert not s[lo:hi].any()
    assert torch.equal(s[:lo], r[:lo]) and torch.equal(s[hi:], r[hi:])
    assert [R.total(p) == 0 for p in R.split_parts(s.numpy(), part_b)] == [k == 1 for k in range(B // part_b)]


# ----------------------------------------------------------------------------- the reference against a loop
def _small(seed, B=3):
    rng = np.random.default_rng(seed)
    set_ = R.random(B, seed).numpy()
    set_[0, 0, 0, 0], set_[B - 1, 31, 25, 25] = True, True
    values = rng.standard_normal(set_.shape).astype(np.float32)
    return values, set_


@pytest.mark.parametrize("part_b", [1, 3])
def test_reference_equals_a_per_element_loop(part_b):
    values, set_ = _small(11)
    loop = R.loop_parts(values, set_, part_b)
    parts = R.split_parts(set_, part_b)
    packed = R.pack_parts(values, set_, part_b)
    assert len(loop) == len(parts) == len(packed) == 3 // part_b
    for k, (p, sk, vk) in enumerate(zip(loop, parts, packed)):
        assert sk.shape == (part_b, 32, 26, 26)
        st = R.stream(sk)
        for name in R.OFFSETS_COLS:
            assert st[name].tolist() == p[name], (k, name)
        assert st["counts"].size == (sk.size + 2047) // 2048 and st["ranks"].size == part_b * R.A_WORDS
        assert vk.dtype == np.float32 and vk.tolist() == p["vals"], k
        assert np.array_equal(R.set_of_words(st["mask"], sk.size), sk.reshape(-1))
        R.assert_stream({n: np.array(p[n]) for n in R.OFFSETS_COLS}, sk)
    # the parts are the chunk's samples in order, each once
    assert np.array_equal(np.concatenate(parts), set_)


@pytest.mark.parametrize("n", [1, 33, 2049])
def test_stream_of_a_ragged_length(n):
    rng = np.random.default_rng(n)
    set_ = rng.random(n) < 0.5
    st = R.stream(set_)
    before = np.cumsum(set_) - set_
    assert np.array_equal(st["ranks"], before[::32]) and np.array_equal(st["offsets"], before[::2048])
    assert st["mask"].size == (n + 31) // 32 and int(st["total"][0]) == int(set_.sum())
    assert np.array_equal(R.set_of_words(st["mask"], n), set_)
    assert not (int(st["mask"][-1]) >> ((n - 1) % 32 + 1))


def test_part_b_must_divide():
    for B, part_b in ((6, 0), (6, 4), (6, -1)):
        with pytest.raises(ValueError, match="must divide"):
            R.check_part_b(B, part_b)
    assert R.check_part_b(6, 3) == 2


def test_column_orders_are_the_headers():
    src = open(os.path.join(ROOT, "include", "slk.h")).read()
    for entry, cols in (("offsets_ranks_parts", R.OFFSETS_COLS), ("unpack_x3_parts", R.UNPACK_COLS),
                        ("dgrad_x3_pack_parts", R.PACK_COLS)):
        m = re.search(r"\*\s+" + entry + r"\s*:\s*\[[^\]]*\]\[(\d)\]\s*=\s*\(([^)]*)\)", src)
        assert m, entry
        assert int(m.group(1)) == len(cols) and tuple(c.strip() for c in m.group(2).split(",")) == cols, entry


# ----------------------------------------------------------------------------- the model and its wrong variants
B9, PB9 = 9, 3


def _degenerate_case():
    set_ = R.degenerate(B9).numpy()
    rng = np.random.default_rng(5)
    values = (rng.integers(1, 1000, set_.shape) * rng.choice([-1, 1], set_.shape)).astype(np.float32)
    return values, set_


def _run_pack(values, set_, part_b, wrong):
    mem, bufs, tots = R.part_memory(values, set_, part_b)
    R.model_pack_parts(values, mem, R.table_rows(R.PACK_COLS, len(bufs), vals="gvals"), part_b, wrong)
    return bufs, tots


def _run_unpack(values, set_, part_b, wrong):
    act = np.where(set_, np.abs(values) + 1, 0).astype(np.float32)
    mem, bufs, _ = R.part_memory(act, set_, part_b)
    return act, R.model_unpack_parts(len(set_), mem, R.table_rows(R.UNPACK_COLS, len(bufs)), part_b, wrong)


def test_model_reproduces_the_reference():
    values, set_ = _degenerate_case()
    for part_b in (1, 3, 9):
        bufs, tots = _run_pack(values, set_, part_b, None)
        want = R.assert_packed_parts(bufs, [1] * len(bufs), values, set_, part_b, "model")
        assert [w.size for w in want] == tots
        act, dense = _run_unpack(values, set_, part_b, None)
        R.assert_unpacked(dense, act, set_, "model")
    values, set_ = _small(13)
    bufs, _ = _run_pack(values, set_, 1, None)
    R.assert_packed_parts(bufs, [1] * 3, values, set_, 1, "model, random")


@pytest.mark.parametrize("wrong", R.WRONG_VARIANTS)
def test_comparisons_refuse_the_wrong_variants(wrong):
    values, set_ = _degenerate_case()
    bufs, _ = _run_pack(values, set_, PB9, wrong)
    with pytest.raises(AssertionError):
        R.assert_packed_parts(bufs, [1] * len(bufs), values, set_, PB9, wrong)
    act, dense = _run_unpack(values, set_, PB9, wrong)
    with pytest.raises(AssertionError):
        R.assert_unpacked(dense, act, set_, wrong)
    # and the mask / rank comparison refuses a rank that counts its own word's first bit
    st = R.stream(set_[:PB9])
    if wrong == "rank_counts_own_bit":
        st["ranks"] = st["ranks"] + (st["mask"] & 1)
        with pytest.raises(AssertionError):
            R.assert_stream(st, set_[:PB9])
    else:
        R.assert_stream(st, set_[:PB9])


def test_comparisons_refuse_a_stray_store():
    values, set_ = _degenerate_case()
    bufs, tots = _run_pack(values, set_, PB9, None)
    for where in (0, 1 + tots[0], bufs[0].size - 1):
        b = [x.copy() for x in bufs]
        b[0][where] = 0.0
        with pytest.raises(AssertionError):
            R.assert_packed_parts(b, [1] * len(b), values, set_, PB9)
