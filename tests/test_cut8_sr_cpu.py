"""The stochastic rounding of the FP8 cut records without a GPU: tests/cut8_sr_ref.py (the host reference of
include/slk.h's "FP8 cut records: stochastic rounding") is pinned by conditions it must meet on its own — the law of the
rounding by enumeration, both-neighbours-only, the strict error bound, idempotence, unbiasedness — and a host build of
csrc/slk_cut8.h is held to it bit for bit; three deliberately wrong variants are shown to fail; plus the refusals of
codec.Fp8Cut(rounding=, seed=) and of the slk_cut8_*_sr entries that need no launch."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cut8_ref as R
import cut8_sr_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [(0, 0, 0), (5, 1, 0), (0xDEADBEEF, 0x80000003, 7)]   # (seed, step, row0); one counter above 2^31


@pytest.fixture(scope="module")
def ref():
    """The generator's set, and per format: nearest records / rows and the stochastic ones under every key."""
    names = [n for n, _ in R.samples()]
    x = R.sample_tensor()
    out = {"names": names, "x": x, "finite": [i for i, n in enumerate(names) if n not in ("has_nan", "has_inf")]}
    for fmt in R.FORMATS:
        rec = R.encode(x, fmt)
        out[fmt] = {"nearest": (rec, R.decode(rec, fmt)[0])}
        for key in KEYS:
            r = S.encode(x, fmt, *key)
            dec, flag = R.decode(r, fmt)
            assert flag == 0
            out[fmt][key] = (r, dec)
    return out


# ------------------------------------------------------------------------------------------------- the law
def _pairs(nb):
    """(rem, s): every rem for s = 1..8, then s = 9..nb and s > nb with chosen 8-bit rems."""
    out = [(rem, s) for s in range(1, 9) for rem in range(1 << s)]
    out += [(rem, s) for s in range(9, nb + 9) for rem in (0, 1, 2, 0x55, 0x80, 0xAA, 0xFF)]
    return out


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_law_by_enumeration_of_the_random_bits(fmt):
    nb = S.NB[fmt]
    assert 16 <= nb <= 21
    space = np.arange(1 << nb, dtype=np.uint32)                  # every pattern of the bits the rule reads
    words = space.astype(np.uint64) << (32 - nb)                 # ... as the top bits of a random word
    low = np.uint64((1 << (32 - nb)) - 1)
    for rem, s in _pairs(nb):
        count = int(S.up_bits(rem / 2.0 ** s, space, nb).sum(dtype=np.int64))
        if s <= nb:
            assert count * (1 << s) == rem * (1 << nb), (rem, s)    # P(up) = rem / 2^s exactly
        else:
            assert count == (rem << nb) >> s, (rem, s)              # floor: below 2^-nb of a quantum too few
            assert 0 <= rem / 2.0 ** s - count / 2.0 ** nb < 2.0 ** -nb
        if rem == 0:
            assert count == 0
        # the bits below the top nb do not matter
        if s in (1, 5, nb):
            assert int(S.up(rem / 2.0 ** s, words, nb).sum(dtype=np.int64)) == count
            assert int(S.up(rem / 2.0 ** s, words | low, nb).sum(dtype=np.int64)) == count


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_law_on_values_with_carry_subnormals_and_below(fmt):
    """|y| = sig * 2^q through split(): the count of round-ups over the bit space is frac * 2^nb, and the upper
    neighbour is the next value of the format — across a binade's top (carry), in the subnormal range, and below
    the smallest subnormal (lower neighbour 0)."""
    _, _, fmax, m, emin = R.FORMATS[fmt]
    nb = S.NB[fmt]
    vals = np.unique(np.abs(R.finite_values(fmt)[0]))
    space = np.arange(1 << nb, dtype=np.uint64) << (32 - nb)
    cases = [(0xFF, -7), (0xFF, emin - 7), (0x81, 0), (0xAB, emin - 9), (0x80, emin - m - 8), (0x01, emin - m - 3),
             (0xFF, emin - m - 12), (0x80, emin - m - 8 - nb), (0xC0, emin - m - 30)]
    for sig, q in cases:
        y = np.array([sig * 2.0 ** q])
        k, frac, quantum = S.split(y, fmt)
        lo_v, hi_v = k[0] * quantum[0], (k[0] + 1) * quantum[0]
        assert lo_v <= y[0] < hi_v and lo_v in vals and hi_v in vals
        assert frac[0] == 0 or list(vals).index(hi_v) == list(vals).index(lo_v) + 1
        count = int(S.up(frac, space, nb).sum(dtype=np.int64))
        assert count == int(np.floor(frac[0] * 2.0 ** nb)), (sig, q)
        if frac[0] * 2.0 ** nb == np.floor(frac[0] * 2.0 ** nb):
            assert count / 2.0 ** nb * quantum[0] + lo_v == y[0]    # the expectation is y itself
    k, frac, quantum = S.split(np.array([0xFF * 2.0 ** -7]), fmt)   # 1.9921875: its upper neighbour is 2.0, a carry
    assert (k[0] + 1) * quantum[0] == 2.0
    k, frac, quantum = S.split(np.array([0x80 * 2.0 ** (emin - m - 8 - 3)]), fmt)
    assert k[0] == 0 and frac[0] == 2.0 ** -4                       # 1/16 of the smallest subnormal


# ---------------------------------------------------------------------------------------- the host build
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        for cand in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
            if os.path.exists(cand):
                cxx = cand
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("cut8_sr_host")
    exe = str(d / "cut8_sr_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "split-learning-k8s_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cut8_sr_host.cc"), "-o", exe], check=True)
    R.to_bits(R.sample_tensor()).tofile(str(d / "in.bin"))

    def run(fmt, seed, step, row0):
        out = str(d / "out.bin")
        subprocess.run([exe, str(d / "in.bin"), out, str(R.FORMATS[fmt][0]), str(seed), str(step), str(row0)], check=True)
        raw = np.fromfile(out, dtype=np.uint8)
        n = raw.size // (R.RECORD + 2 * R.SAMPLE)
        return raw[:n * R.RECORD].reshape(n, R.RECORD), raw[n * R.RECORD:].view(np.uint16).reshape(n, R.SAMPLE)
    return run


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_header_agrees_with_the_reference(ref, host, fmt):
    for key in KEYS:
        rec, dec = host(fmt, *key)
        want_rec, want_dec = ref[fmt][key]
        assert np.array_equal(rec, want_rec), key
        assert np.array_equal(dec, R.to_bits(want_dec)), key


# ------------------------------------------------------------------------------------- checks on the results
def _neighbours_only(x, rec, fmt, rows):
    """Every code's value is one of the two format values around y, with x's sign."""
    vals = np.unique(np.abs(R.finite_values(fmt)[0]))
    e = R.record_e(rec)[rows].astype(np.float64)[:, None]
    y = x[rows].double().numpy() * 2.0 ** -e
    got = torch.from_numpy(rec[rows, R.HEADER:].copy()).view(R.FORMATS[fmt][1]).float().double().numpy()
    lo = vals[np.searchsorted(vals, np.abs(y), side="right") - 1]
    hi = vals[np.minimum(np.searchsorted(vals, np.abs(y), side="left"), len(vals) - 1)]
    ok = ((np.abs(got) == lo) | (np.abs(got) == hi)) & (np.signbit(got) == np.signbit(y))
    return bool(ok.all())


def _strict_bound(x, dec, rec, fmt, rows):
    _, _, _, m, emin = R.FORMATS[fmt]
    xv, xh = x[rows].double().numpy(), dec[rows].double().numpy()
    e = R.record_e(rec)[rows].astype(np.float64)[:, None]
    bound = np.maximum(np.abs(xv) * 2.0 ** -m, 2.0 ** e * 2.0 ** (emin - m))
    return bool(np.isfinite(xh).all() and (np.abs(xv - xh) < bound).all())


def _idempotent(ref, fmt, encode):
    """Values that nearest rounding reproduces are fixed points, bit for bit, for any key. The one decoded value that
    is not such a value is the saturated top of bf16's range, 255 * 2^120 (0x7F7F: eight significant bits, written
    where a finite code's product reaches 2^128): it is excluded here and goes to either of its neighbours."""
    fixed = ref[fmt]["nearest"][1]
    top = (R.to_bits(fixed) & 0x7fff) == 0x7f7f
    assert top.any()
    for key in KEYS:
        again = R.to_bits(R.decode(encode(fixed, fmt, *key), fmt)[0])
        if not np.array_equal(again[~top], R.to_bits(fixed)[~top]):
            return False
        assert np.isin(again[top] & 0x7fff, (0x7f7f, 0x7f70 if fmt == "e4m3" else 0x7f60)).all()
    return True


def _unbiased_row(ref):
    row = ref["x"][ref["names"].index(S.UNBIASED_SAMPLE)]
    return row[None].expand(S.UNBIASED_ROWS, R.SAMPLE).contiguous()


def _unbiased(ref, fmt, variant=None):
    x = _unbiased_row(ref)
    seed, step = S.UNBIASED_KEY
    mean = S.roundtrip(x, fmt, seed, step, 0, variant).double().numpy().mean(axis=0)
    dev = np.abs(mean - x[0].double().numpy()) / S.quanta(x[:1], fmt)[0]
    return float(dev.max())


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_both_neighbours_only_and_strict_bound(ref, fmt):
    rows = ref["finite"]
    moved = 0
    for key in KEYS:
        rec, dec = ref[fmt][key]
        assert _neighbours_only(ref["x"], rec, fmt, rows)
        assert _strict_bound(ref["x"], dec, rec, fmt, rows)
        assert np.array_equal(rec[:, :R.HEADER], ref[fmt]["nearest"][0][:, :R.HEADER])   # e, fmt, reserved: unchanged
        moved += int((rec != ref[fmt]["nearest"][0]).sum())
        for n in ("has_nan", "has_inf"):                                                 # poisoned as in the nearest entries
            i = ref["names"].index(n)
            assert R.record_e(rec)[i] == R.POISON and not rec[i, R.HEADER:].any()
        z = ref["names"].index("all_zero")
        assert R.record_e(rec)[z] == 0 and not rec[z, R.HEADER:].any()
    assert moved > 0
    a, b = ref[fmt][KEYS[0]][0], ref[fmt][KEYS[1]][0]
    assert (a != b).any()                                                                # the key matters


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_zero_keeps_its_sign_and_nearest_fixed_points_stay(ref, fmt):
    assert _idempotent(ref, fmt, S.encode)
    for key in KEYS:
        codes = S.encode(_tiny(fmt), fmt, *key)[0, R.HEADER:]
        assert codes[0] == 0x78                                      # 1.0 * 2^-e = 2^8 | 2^15: field 15 << 3 | 30 << 2
        neg, pos = codes[1:2001], codes[2001:4001]
        assert set(neg.tolist()) == {0x80, 0x81} and set(pos.tolist()) == {0x00, 0x01}   # a zero keeps x's sign
        assert 350 < int((neg == 0x81).sum()) < 650 and 350 < int((pos == 0x01).sum()) < 650   # P(up) = 1/4, 6 sigma


def _tiny(fmt):
    """One sample: 1.0, then 2000 times -1/4 and 2000 times +1/4 of the smallest subnormal's value under its e."""
    e = {"e4m3": -8, "e5m2": -15}[fmt]
    _, _, _, m, emin = R.FORMATS[fmt]
    x = torch.zeros(1, R.SAMPLE, dtype=torch.bfloat16)
    x[0, 0] = 1.0
    x[0, 1:2001] = -(2.0 ** (e + emin - m - 2))
    x[0, 2001:4001] = 2.0 ** (e + emin - m - 2)
    return x


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_slices_encode_to_the_rows_of_the_whole(ref, fmt):
    seed, step, _ = KEYS[1]
    whole = S.encode(ref["x"][:5], fmt, seed, step, 0)
    assert np.array_equal(S.encode(ref["x"][2:5], fmt, seed, step, 2), whole[2:5])
    assert (S.encode(ref["x"][2:5], fmt, seed, step, 0) != whole[2:5]).any()


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_unbiased_within_the_hoeffding_bound(ref, fmt):
    assert _unbiased(ref, fmt) <= S.UNBIASED_T


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_three_wrong_variants_are_visible(ref, host, fmt):
    # nearest rounding and truncation are biased: both leave the Hoeffding bound (and nearest is not what the host build gives)
    assert _unbiased(ref, fmt, "nearest") > S.UNBIASED_T
    assert _unbiased(ref, fmt, "truncate") > S.UNBIASED_T
    # one word per row passes every per-element check, but it is not the header's rule
    key = KEYS[1]
    shared = S.encode(ref["x"], fmt, *key, variant="shared_word")
    assert _neighbours_only(ref["x"], shared, fmt, ref["finite"])
    assert not np.array_equal(host(fmt, *key)[0], shared)
    # ... and its elements move together: where a row holds one value many times, the copies all go the same way
    x = torch.full((4, R.SAMPLE), 1.0 + 2.0 ** -6, dtype=torch.bfloat16)
    x[:, 0] = 1.75
    for variant, spread in (("shared_word", False), (None, True)):
        codes = S.encode(x, fmt, *key, variant=variant)[:, R.HEADER + 1:]
        assert all((len(np.unique(row)) > 1) == spread for row in codes)


# ------------------------------------------------------------------------------------------ refusals
def test_fp8cut_rounding_argument():
    from splitcnn.codec import Fp8Cut
    q = Fp8Cut()
    assert q.rounding_of("fwd") == "nearest" and q.rounding_of("bwd") == "nearest" and q.seed == 0
    assert "rounding='nearest'" in repr(q) and q.nearest() is q
    q = Fp8Cut(rounding="stochastic", seed=5)
    assert q.rounding_of("fwd") == "stochastic" and q.rounding_of("bwd") == "stochastic"
    assert "rounding='stochastic'" in repr(q) and "seed=5" in repr(q)
    q = Fp8Cut(rounding={"bwd": "stochastic"})
    assert q.rounding_of("fwd") == "nearest" and q.rounding_of("bwd") == "stochastic" and "'bwd': 'stochastic'" in repr(q)
    n = q.nearest()
    assert n is q.nearest() and (n.fwd, n.bwd) == (q.fwd, q.bwd) and n.rounding_of("bwd") == "nearest"
    assert Fp8Cut(fwd=None, rounding={"bwd": "stochastic"}).rounding_of("bwd") == "stochastic"
    assert not hasattr(q, "set_rounding") and not hasattr(q, "set_seed")
    for bad in ("random", "Stochastic", None, 1, {"bwd": "sr"}, {"fwd": None}):
        with pytest.raises(ValueError, match="expected one of"):
            Fp8Cut(rounding=bad)
    with pytest.raises(ValueError, match="keys"):
        Fp8Cut(rounding={"both": "stochastic"})
    with pytest.raises(ValueError, match="dense"):
        Fp8Cut(bwd=None, rounding={"bwd": "stochastic"})
    with pytest.raises(ValueError, match="dense"):
        Fp8Cut(fwd=None, rounding="stochastic")
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            Fp8Cut(seed=bad)
    with pytest.raises(ValueError, match="direction"):
        q.rounding_of("sideways")
    x = torch.zeros(2, R.SAMPLE, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.roundtrip(x, x, "bwd", step=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.encode(x, torch.zeros(2, R.RECORD, dtype=torch.uint8), "bwd", step=torch.zeros(1, dtype=torch.int32))


def test_sr_entry_points_validate_without_gpu():
    from splitcnn import _lib
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: refused before any use
    for name in ("slk_cut8_encode_sr", "slk_cut8_roundtrip_sr"):
        fn = getattr(lib, name)
        for fmt in (0, 1):
            assert fn(None, -1, fmt, None, 0, None, 0, None) == 1      # hipErrorInvalidValue
            assert fn(None, 0, fmt, None, 0, None, 0, None) == 0       # empty: no launch
            assert fn(None, 0, fmt, None, 0, None, -1, None) == 1      # row0 < 0, even when empty
            assert fn(None, 2, fmt, p, 0, p, 0, None) == 1             # null pointers
            assert fn(p, 2, fmt, None, 0, p, 0, None) == 1
            assert fn(p, 2, fmt, p, 0, None, 0, None) == 1             # no step
            assert fn(p + 2, 1, fmt, p, 0, p, 0, None) == 1            # misaligned
            assert fn(p, 1, fmt, p + 8, 0, p, 0, None) == 1
            assert fn(p, 1, fmt, p, 0, p + 2, 0, None) == 1            # step: 4-byte alignment
            assert fn(p, 1, fmt, p, 0, p, -1, None) == 1               # row0 < 0
        for fmt in (-1, 2):
            assert fn(p, 1, fmt, p, 0, p, 0, None) == 1
            assert fn(None, 0, fmt, None, 0, None, 0, None) == 1
