"""The FP8 cut record rule without a GPU: tests/cut8_ref.py (the host reference of include/slk.h's "FP8 cut records")
and its input generator are pinned by conditions they must meet on their own — the GPU tests then hold the kernels to
this reference bit for bit — plus the refusals of codec.Fp8Cut, of the slk_cut8_* entries and of dist.WideHub(codec=)
that need no launch."""
import types

import numpy as np
import pytest
import torch

import cut8_ref as R


@pytest.fixture(scope="module")
def ref():
    """The generator's set with the reference's records and decoded rows, computed once per format."""
    names = [n for n, _ in R.samples()]
    x = R.sample_tensor()
    out = {"names": names, "x": x}
    for fmt in R.FORMATS:
        rec = R.encode(x, fmt)
        dec, flag = R.decode(rec, fmt)
        assert flag == 0
        out[fmt] = (rec, dec)
    return out


def _finite_rows(ref):
    return [i for i, n in enumerate(ref["names"]) if n not in ("has_nan", "has_inf")]


def test_generator_covers_the_listed_cases(ref):
    names, bits = ref["names"], R.to_bits(ref["x"])
    amax = (bits & 0x7fff).max(axis=1)
    for man in (0x00, 0x60, 0x61, 0x7f):
        assert sum(1 for i, n in enumerate(names) if n.startswith("amax_") and (amax[i] & 0x7f) == man) >= 3
    i = names.index("subnormal_amax")
    assert 0 < amax[i] < 0x80
    assert any(0 < float(R.from_bits(amax[j:j + 1]).double()) < 2.0 ** -100 and amax[j] >= 0x80 for j in range(len(names)))
    assert 0x7f7f in amax                                   # the largest finite bf16
    assert not bits[names.index("all_zero")].any()
    assert not (bits[names.index("non_negative")] & 0x8000).any()
    wide = bits[names.index("amax_ex127_man00")]
    mag = wide & 0x7fff
    assert (wide & 0x8000).any() and (~wide & 0x8000).any() and int(mag.max() >> 7) - int(mag[mag > 0].min() >> 7) >= 20
    assert torch.isnan(ref["x"][names.index("has_nan")].float()).sum() == 1
    assert torch.isinf(ref["x"][names.index("has_inf")].float()).sum() == 1


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_exponent_is_minimal_and_header_is_as_specified(ref, fmt):
    word, _, fmax, _, _ = R.FORMATS[fmt]
    rec, _ = ref[fmt]
    assert rec.shape == (len(ref["names"]), 16400) and R.RECORD == 16400
    e = R.record_e(rec)
    assert (np.ascontiguousarray(rec[:, 4:8]).view(np.uint32).reshape(-1) == word).all() and not rec[:, 8:16].any()
    amax = ref["x"].float().abs().max(dim=1).values.double().numpy()
    clamped = 0
    for i in _finite_rows(ref):
        if amax[i] == 0:
            assert e[i] == 0
            continue
        assert -100 <= e[i] <= 127 and amax[i] * 2.0 ** -int(e[i]) <= fmax
        if e[i] > -100:
            assert amax[i] * 2.0 ** -(int(e[i]) - 1) > fmax, ref["names"][i]
        else:
            clamped += 1
    assert clamped >= 2 and len(set(e[_finite_rows(ref)].tolist())) >= 8
    # neither format's NaN / inf codes are produced
    vals = torch.from_numpy(rec[_finite_rows(ref), 16:].copy()).view(R.FORMATS[fmt][1]).float()
    assert bool(torch.isfinite(vals).all())


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_error_bound_in_float64(ref, fmt):
    _, _, _, m, emin = R.FORMATS[fmt]
    rec, dec = ref[fmt]
    rows = _finite_rows(ref)
    x, xh = ref["x"][rows].double().numpy(), dec[rows].double().numpy()
    e = R.record_e(rec)[rows].astype(np.float64)[:, None]
    bound = np.maximum(np.abs(x) * 2.0 ** -(m + 1), 2.0 ** e * 2.0 ** (emin - m - 1))
    assert np.isfinite(xh).all()   # a finite sample stays finite (the top of bf16's range saturates)
    assert (np.abs(x - xh) <= bound).all()
    assert (np.abs(x - xh) > 0).any()   # lossy: the bound is not vacuous


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_roundtrip_is_idempotent_in_decoded_bits(ref, fmt):
    _, dec = ref[fmt]
    again = R.roundtrip(dec, fmt)
    assert np.array_equal(R.to_bits(again), R.to_bits(dec))


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_every_finite_code_and_exact_ties_occur(ref, fmt):
    rec, _ = ref[fmt]
    rows = _finite_rows(ref)
    vals, codes = R.finite_values(fmt)
    assert len(codes) == {"e4m3": 254, "e5m2": 248}[fmt] and 0x00 in codes and 0x80 in codes
    seen = np.unique(rec[rows, 16:])
    assert np.array_equal(seen, np.sort(codes))
    # exact ties: y = x 2^-e halfway between two neighbouring values; the even code (low mantissa bit 0) wins
    pos = np.unique(np.abs(vals))
    mids = (pos[:-1] + pos[1:]) / 2
    e = R.record_e(rec)[rows].astype(np.float64)[:, None]
    y = np.abs(ref["x"][rows].double().numpy()) * 2.0 ** -e
    tie = np.isin(y, mids)
    assert tie.sum() >= len(mids)
    assert not (rec[rows, 16:][tie] & 1).any()


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_poisoned_and_malformed_records(ref, fmt):
    rec, dec = ref[fmt]
    names = ref["names"]
    for n in ("has_nan", "has_inf"):
        i = names.index(n)
        assert R.record_e(rec)[i] == 0x7FFFFFFF and not rec[i, 16:].any()
        assert (R.to_bits(dec[i]) == 0x7FC0).all()
    good = names.index("amax_ex127_man61")
    for kind in R.MALFORMED:
        three = np.stack([rec[good], R.malform(rec[good], kind), rec[good + 1]])
        out, flag = R.decode(three, fmt)
        assert flag == 1
        assert (R.to_bits(out[1]) == 0x7FC0).all()
        assert np.array_equal(R.to_bits(out[0]), R.to_bits(dec[good]))
        assert np.array_equal(R.to_bits(out[2]), R.to_bits(dec[good + 1]))
    other = [f for f in R.FORMATS if f != fmt][0]
    assert R.decode(rec[good:good + 1], other)[1] == 1   # the other format's record is malformed here


def test_fp8cut_constructor_refusals():
    from splitcnn.codec import CUT8_RECORD, CUT8_SAMPLE, Fp8Cut
    assert (CUT8_SAMPLE, CUT8_RECORD) == (R.SAMPLE, R.RECORD)
    q = Fp8Cut()
    assert (q.fwd, q.bwd) == ("e4m3", "e5m2") and q.format("fwd") == "e4m3" and q.format("bwd") == "e5m2"
    assert Fp8Cut(fwd=None).format("fwd") is None and Fp8Cut(bwd=None, fwd="e5m2").fwd == "e5m2"
    with pytest.raises(ValueError, match="both None"):
        Fp8Cut(fwd=None, bwd=None)
    for kw in ({"fwd": "e3m4"}, {"bwd": "fp8"}, {"fwd": 0}):
        with pytest.raises(ValueError, match="expected one of"):
            Fp8Cut(**kw)
    with pytest.raises(ValueError, match="direction"):
        q.format("sideways")
    with pytest.raises(ValueError, match="dense"):
        Fp8Cut(bwd=None).roundtrip(torch.zeros(1), torch.zeros(1), "bwd")
    x = torch.zeros(2, 32, 8, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.roundtrip(x, x, "fwd")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.encode(x, torch.zeros(2, CUT8_RECORD, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.decode(torch.zeros(2, CUT8_RECORD, dtype=torch.uint8), x, torch.zeros(1, dtype=torch.int32))


def test_entry_points_validate_without_gpu():
    from splitcnn import _lib
    lib = _lib.load()
    assert lib.slk_cut8_record_bytes() == 16400
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16   # a 16-byte aligned host address: refused before any use
    for fmt in (0, 1):
        assert lib.slk_cut8_encode(None, -1, fmt, None, None) == 1      # hipErrorInvalidValue
        assert lib.slk_cut8_decode(None, -1, fmt, None, None, None) == 1
        assert lib.slk_cut8_roundtrip(None, -1, fmt, None, None) == 1
        assert lib.slk_cut8_encode(None, 0, fmt, None, None) == 0       # empty: no launch
        assert lib.slk_cut8_decode(None, 0, fmt, None, None, None) == 0
        assert lib.slk_cut8_roundtrip(None, 0, fmt, None, None) == 0
        assert lib.slk_cut8_encode(None, 2, fmt, p, None) == 1          # null pointers
        assert lib.slk_cut8_decode(p, 2, fmt, p, None, None) == 1       # no err_flag
        assert lib.slk_cut8_roundtrip(p, 2, fmt, None, None) == 1
        assert lib.slk_cut8_encode(p + 2, 1, fmt, p, None) == 1         # misaligned
        assert lib.slk_cut8_encode(p, 1, fmt, p + 8, None) == 1
        assert lib.slk_cut8_decode(p, 1, fmt, p + 4, p, None) == 1
        assert lib.slk_cut8_decode(p, 1, fmt, p, p + 2, None) == 1
        assert lib.slk_cut8_roundtrip(p, 1, fmt, p + 2, None) == 1
    for fmt in (-1, 2):
        assert lib.slk_cut8_encode(p, 1, fmt, p, None) == 1
        assert lib.slk_cut8_decode(p, 1, fmt, p, p, None) == 1
        assert lib.slk_cut8_roundtrip(p, 1, fmt, p, None) == 1
        assert lib.slk_cut8_roundtrip(None, 0, fmt, None, None) == 1


def test_widehub_refuses_codec_on_a_cpu_stage():
    from splitcnn.codec import Fp8Cut
    from splitcnn.dist import WideHub
    stage = types.SimpleNamespace(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="CUDA"):
        WideHub(stage, 0, 3, groups=(None, None), codec=Fp8Cut())
    with pytest.raises(TypeError, match="Fp8Cut"):
        WideHub(stage, 0, 3, groups=(None, None), codec="e4m3")
    hub = WideHub(stage, 0, 3, groups=(None, None))   # no codec: as before
    assert hub.codec is None and hub.err_flag is None and hub.dense_bytes == 0
    hub.check_exchange()


def test_wide_trainer_refuses_a_foreign_codec():
    from splitcnn.codec import check_cut_codec, Fp8Cut
    assert check_cut_codec(None) is None
    q = Fp8Cut()
    assert check_cut_codec(q) is q
    with pytest.raises(TypeError, match="Fp8Cut"):
        check_cut_codec(object())
