"""Lossless sparse codec for the multi-GPU cut exchange (csrc/slk_codec.hip).

The reference ships the dense fp32 cut and the dense fp32 cut gradient (src/client_part.py:117-125,
src/server_part.py:57-58). The cut is a ReLU output, so on the RCCL path a micro-batch travels as a
bit mask of its nonzero elements plus those elements in order, and the gradient as its values at the
same positions only: the client applies its own ReLU mask before using the gradient (ReLU's backward
in activations.backward, src/client_part.py:132), so the positions left out never reach a result.
Every weight, loss and gradient downstream is bit-identical to the dense exchange.

The widened model's bf16 cut (K5, wide.py) has a codec of its own, Fp8Cut (csrc/slk_cut8.hip): opt-in and lossy, one
power-of-two scale per sample and OCP FP8 codes, half the bytes in each direction; and a block-scaled one, MxCut
(csrc/slk_cutmx.hip): one E8M0 scale per 32 elements and OCP e2m1 / e4m3 codes, 0.27 / 0.52 of the bytes.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import _dev, _stream

CUT8_SAMPLE = 16384      # bf16 elements of one K5 cut [256,8,8] or of one cut-gradient row
CUT8_RECORD = 16400      # bytes of one record: a 16-byte header and one fp8 code per element
CUT8_FORMATS = {"e4m3": 0, "e5m2": 1}
CUT8_ROUNDINGS = ("nearest", "stochastic")
CUTMX_BLOCK = 32         # elements under one scale byte of an MX record
CUTMX_FORMATS = {"e2m1": 0, "e4m3": 1}
CUTMX_RECORD = {"e2m1": 8720, "e4m3": 16912}   # a 16-byte header, 512 scale bytes, 4- or 8-bit codes


class CutCodec:
    """Per micro-batch encode / offsets / pack / unpack over caller-visible buffers (one set per key)."""

    def __init__(self):
        self._bufs = {}

    def _buf(self, key, shape, dtype, device):
        # keyed by shape too: a buffer is never replaced, so a HIP graph captured around these kernels at
        # one micro-batch size keeps valid pointers after another size has run (dist.Hub's chunk graphs)
        k = (key, tuple(shape), dtype, str(torch.device(device)))
        t = self._bufs.get(k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=device)
            self._bufs[k] = t
        return t

    def buffers(self, key, n: int, device):
        """(mask words, counts, offsets, total[1], vals[n]) for a micro-batch of n elements."""
        nb = _lib.query("slk_cut_blocks", n)
        return (self._buf((key, "mask"), ((n + 31) // 32,), torch.int32, device),
                self._buf((key, "counts"), (nb,), torch.int32, device),
                self._buf((key, "offsets"), (nb,), torch.int32, device),
                self._buf((key, "total"), (1,), torch.int32, device),
                self._buf((key, "vals"), (n,), torch.float32, device))

    def ranks_buffer(self, key, n: int, device):
        """The word-ranks buffer of key's micro-batch (int32, ceil(n/32)), not computed."""
        return self._buf((key, "ranks"), ((n + 31) // 32,), torch.int32, device)

    def ranks(self, key, n: int, bufs):
        """Word ranks of a micro-batch whose offsets are computed (offsets() / encode()): ranks[w] = the vals
        index of mask word w's first set element, for the fused consumers (ops.cut_unpack_x3,
        ops.conv2_dgrad_x3_pack). Buffer keyed like buffers()."""
        mask, _, offsets, _, _ = bufs
        r = self.ranks_buffer(key, n, mask.device)
        _lib.call("slk_cut_ranks", mask.data_ptr(), n, offsets.data_ptr(), r.data_ptr(), _stream(mask))
        return r

    @staticmethod
    def encode(x, bufs):
        mask, counts, offsets, total, vals = bufs
        _lib.call("slk_cut_encode", x.data_ptr(), x.numel(), mask.data_ptr(), counts.data_ptr(), offsets.data_ptr(),
                  total.data_ptr(), vals.data_ptr(), _stream(x))

    @staticmethod
    def offsets(n: int, bufs):
        mask, counts, offsets, total, _ = bufs
        _lib.call("slk_cut_offsets", mask.data_ptr(), n, counts.data_ptr(), offsets.data_ptr(), total.data_ptr(),
                  _stream(mask))

    @staticmethod
    def pack(x, bufs, vals=None):
        mask, _, offsets, _, v = bufs
        v = v if vals is None else vals
        _lib.call("slk_cut_pack", x.data_ptr(), x.numel(), mask.data_ptr(), offsets.data_ptr(), v.data_ptr(), _stream(x))

    @staticmethod
    def unpack(out, bufs, vals=None):
        mask, _, offsets, _, v = bufs
        v = v if vals is None else vals
        _lib.call("slk_cut_unpack", v.data_ptr(), out.numel(), mask.data_ptr(), offsets.data_ptr(), out.data_ptr(),
                  _stream(out))


class Fp8Cut:
    """Opt-in lossy FP8 exchange of the widened model's cut (csrc/slk_cut8.hip; the rule is in include/slk.h,
    "FP8 cut records"): one power-of-two scale per sample, OCP fp8 codes, 16,400 bytes a sample against the bf16
    cut's 32,768. `fwd` is the format of the cut ("e4m3" by convention), `bwd` that of the cut gradient ("e5m2");
    either may be None, which leaves that direction dense bf16. The formats are constructor constants passed to the
    kernels by value: a captured graph keeps them, and there is no setter.

    `rounding` is "nearest" (round to nearest even), "stochastic", or a dict per direction such as
    {"bwd": "stochastic"} (a missing key means nearest). A stochastic direction sends every element to one of its two
    neighbouring codes with probabilities that make the expectation equal to the value (include/slk.h, "FP8 cut records:
    stochastic rounding"), under a random word keyed on (`seed`, a device step counter, the global row row0 + row,
    the element): its encode / roundtrip take `step`, a device int32[1] the kernel reads at run time — a captured
    graph follows it — and `row0`, the global row of the first sample, so a slice of a batch encodes to the bits of
    the whole batch. `rounding` and `seed` are constructor constants passed to the kernels by value like the formats:
    a captured graph keeps them, and there is no setter. decode does not depend on the rounding.

    A sample is 16,384 contiguous bf16 elements: x / out are [n, ...] with 16,384 elements per row, records are
    uint8 [n, 16400]. Every method works on caller-visible buffers and launches on the tensor's current stream."""

    def __init__(self, fwd="e4m3", bwd="e5m2", rounding="nearest", seed: int = 0):
        for name, v in (("fwd", fwd), ("bwd", bwd)):
            if v is not None and v not in CUT8_FORMATS:
                raise ValueError(f"Fp8Cut: {name}={v!r}; expected one of {sorted(CUT8_FORMATS)} or None")
        if fwd is None and bwd is None:
            raise ValueError("Fp8Cut: fwd and bwd are both None — that is the dense exchange (pass no codec)")
        self.fwd, self.bwd = fwd, bwd
        if isinstance(rounding, dict):
            extra = sorted(set(rounding) - {"fwd", "bwd"}, key=repr)
            if extra:
                raise ValueError(f"Fp8Cut: rounding has keys {extra}; expected 'fwd' and / or 'bwd'")
            rounding = {d: rounding.get(d, "nearest") for d in ("fwd", "bwd")}
        else:
            rounding = {"fwd": rounding, "bwd": rounding}
        for d, v in rounding.items():
            if not isinstance(v, str) or v not in CUT8_ROUNDINGS:
                raise ValueError(f"Fp8Cut: rounding of {d} is {v!r}; expected one of {list(CUT8_ROUNDINGS)}")
            if v == "stochastic" and self.format(d) is None:
                raise ValueError(f"Fp8Cut: rounding of {d} is 'stochastic' but {d}=None leaves that direction dense; "
                                 f"name the other direction alone: rounding={{'{'bwd' if d == 'fwd' else 'fwd'}': "
                                 "'stochastic'}")
        self._rounding = rounding
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"Fp8Cut: seed={seed!r}; expected an integer in [0, 2^32)")
        self.seed = seed
        self._nearest = None
        self._bufs = {}

    def __repr__(self):
        r = self._rounding
        shown = r["fwd"] if r["fwd"] == r["bwd"] else r
        return f"Fp8Cut(fwd={self.fwd!r}, bwd={self.bwd!r}, rounding={shown!r}, seed={self.seed})"

    def rounding_of(self, direction: str) -> str:
        """The rounding of "fwd" / "bwd": "nearest" or "stochastic"."""
        self.format(direction)
        return self._rounding[direction]

    def nearest(self) -> "Fp8Cut":
        """This codec's formats with round-to-nearest in both directions (what evaluation uses): self if it is that
        already, otherwise one twin kept for the codec's lifetime, so its buffers stay valid under a captured graph."""
        if all(v == "nearest" for v in self._rounding.values()):
            return self
        if self._nearest is None:
            self._nearest = Fp8Cut(self.fwd, self.bwd)
        return self._nearest

    def format(self, direction: str):
        """The format name of "fwd" / "bwd", or None where that direction stays dense."""
        if direction not in ("fwd", "bwd"):
            raise ValueError(f"Fp8Cut: direction {direction!r}; expected 'fwd' or 'bwd'")
        return self.fwd if direction == "fwd" else self.bwd

    def _fmt(self, direction: str) -> int:
        name = self.format(direction)
        if name is None:
            raise ValueError(f"Fp8Cut: the {direction} direction is dense (built with {direction}=None)")
        return CUT8_FORMATS[name]

    @staticmethod
    def _rows(t, name) -> int:
        """Checked sample count of a bf16 tensor [n, ...] of 16,384 elements per row."""
        _dev(t, name, dtype=torch.bfloat16)
        if t.dim() < 1 or t.numel() != t.shape[0] * CUT8_SAMPLE:
            raise ValueError(f"{name}: expected [n, ...] with {CUT8_SAMPLE} elements per sample, got {tuple(t.shape)}")
        Fp8Cut._aligned(t, name)
        return int(t.shape[0])

    @staticmethod
    def _records(rec, n, name="rec"):
        _dev(rec, name, (n, CUT8_RECORD), torch.uint8)
        Fp8Cut._aligned(rec, name)

    @staticmethod
    def _aligned(t, name):
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: the base address must be 16-byte aligned")

    def record_bytes(self, direction: str) -> int:
        """Bytes of one sample's record in "fwd" / "bwd": 16,400 in either format."""
        self._fmt(direction)
        return CUT8_RECORD

    def records(self, key, n: int, device, direction=None):
        """The uint8 [n, 16400] record buffer of `key`. Keyed by shape too and never replaced, so a HIP graph
        captured around the kernels at one size keeps valid pointers after another size has run (CutCodec._buf).
        `direction` is accepted for MxCut's sake and ignored: both formats have one record width."""
        k = (key, int(n), str(torch.device(device)))
        t = self._bufs.get(k)
        if t is None:
            t = torch.empty((int(n), CUT8_RECORD), dtype=torch.uint8, device=device)
            self._bufs[k] = t
        return t

    def _key(self, direction, x, step, row0):
        """(seed, step pointer, row0) of a stochastic launch, checked; None where `direction` rounds to nearest."""
        if self.rounding_of(direction) != "stochastic":
            return None
        if step is None:
            raise ValueError(f"Fp8Cut: the {direction} direction rounds stochastically and needs step=, a device "
                             "int32[1] counter (a stage's step_ctr)")
        _dev(step, "step", (1,), torch.int32)
        if step.device != x.device:
            raise ValueError(f"step: on {step.device}, the tensor is on {x.device}")
        if isinstance(row0, bool) or not isinstance(row0, int) or not 0 <= row0 < 2 ** 31:
            raise ValueError(f"row0={row0!r}; expected an integer in [0, 2^31)")
        return self.seed, step.data_ptr(), row0

    def encode(self, x, rec, direction: str = "fwd", step=None, row0: int = 0):
        """x (bf16 [n, ...]) -> rec (uint8 [n, 16400]) in `direction`'s format and rounding; a stochastic direction
        needs `step` (device int32[1]) and takes `row0`, the global row of x[0]."""
        fmt, n = self._fmt(direction), self._rows(x, "x")
        self._records(rec, n)
        key = self._key(direction, x, step, row0)
        if key is None:
            _lib.call("slk_cut8_encode", x.data_ptr(), n, fmt, rec.data_ptr(), _stream(x))
        else:
            _lib.call("slk_cut8_encode_sr", x.data_ptr(), n, fmt, rec.data_ptr(), *key, _stream(x))
        return rec

    def decode(self, rec, out, err_flag, direction: str = "fwd"):
        """rec -> out (bf16 [n, ...]); a malformed record (not `direction`'s format, a nonzero reserved word, an
        exponent out of range) decodes to NaNs and sets err_flag (int32 [1])."""
        fmt, n = self._fmt(direction), self._rows(out, "out")
        self._records(rec, n)
        _dev(err_flag, "err_flag", (1,), torch.int32)
        _lib.call("slk_cut8_decode", rec.data_ptr(), n, fmt, out.data_ptr(), err_flag.data_ptr(), _stream(out))
        return out

    def roundtrip(self, x, out, direction: str, step=None, row0: int = 0):
        """out = decode(encode(x)) bit for bit in one launch, no record in memory; out may be x. `step` and `row0`
        as for encode."""
        fmt, n = self._fmt(direction), self._rows(x, "x")
        if self._rows(out, "out") != n:
            raise ValueError(f"out: expected {n} samples like x, got {out.shape[0]}")
        key = self._key(direction, x, step, row0)
        if key is None:
            _lib.call("slk_cut8_roundtrip", x.data_ptr(), n, fmt, out.data_ptr(), _stream(x))
        else:
            _lib.call("slk_cut8_roundtrip_sr", x.data_ptr(), n, fmt, out.data_ptr(), *key, _stream(x))
        return out


class MxCut:
    """Opt-in lossy block-scaled exchange of the widened model's cut (csrc/slk_cutmx.hip; the rule is in
    include/slk.h, "MX cut records"): one E8M0 power-of-two scale per 32 consecutive elements and OCP codes — "e2m1"
    (FP4, 8,720 bytes a sample) or "e4m3" (16,912) against the bf16 cut's 32,768. `fwd` is the format of the cut, `bwd`
    that of the cut gradient; either may be None, which leaves that direction dense bf16. The formats are constructor
    constants passed to the kernels by value: a captured graph keeps them, and there is no setter. Rounding is to
    nearest even only (rounding_of is always "nearest"; there is no rounding= parameter).

    A sample is 16,384 contiguous bf16 elements: x / out are [n, ...] with 16,384 elements per row, records are uint8
    [n, record_bytes(direction)]. The surface is Fp8Cut's: every method works on caller-visible buffers and launches on
    the tensor's current stream; encode / roundtrip accept and ignore step= / row0= (the hub passes them to every
    codec)."""

    def __init__(self, fwd="e2m1", bwd="e4m3"):
        for name, v in (("fwd", fwd), ("bwd", bwd)):
            if v is not None and v not in CUTMX_FORMATS:
                raise ValueError(f"MxCut: {name}={v!r}; expected one of {sorted(CUTMX_FORMATS)} or None")
        if fwd is None and bwd is None:
            raise ValueError("MxCut: fwd and bwd are both None — that is the dense exchange (pass no codec)")
        self.fwd, self.bwd = fwd, bwd
        self._bufs = {}

    def __repr__(self):
        return f"MxCut(fwd={self.fwd!r}, bwd={self.bwd!r})"

    def rounding_of(self, direction: str) -> str:
        """The rounding of "fwd" / "bwd": always "nearest"."""
        self.format(direction)
        return "nearest"

    def nearest(self) -> "MxCut":
        """This codec (what evaluation uses): it rounds to nearest already."""
        return self

    def format(self, direction: str):
        """The format name of "fwd" / "bwd", or None where that direction stays dense."""
        if direction not in ("fwd", "bwd"):
            raise ValueError(f"MxCut: direction {direction!r}; expected 'fwd' or 'bwd'")
        return self.fwd if direction == "fwd" else self.bwd

    def _name(self, direction: str) -> str:
        name = self.format(direction)
        if name is None:
            raise ValueError(f"MxCut: the {direction} direction is dense (built with {direction}=None)")
        return name

    def record_bytes(self, direction: str) -> int:
        """Bytes of one sample's record in "fwd" / "bwd": 8,720 (e2m1) or 16,912 (e4m3)."""
        return CUTMX_RECORD[self._name(direction)]

    def _records(self, rec, n, direction, name="rec"):
        _dev(rec, name, (n, self.record_bytes(direction)), torch.uint8)
        Fp8Cut._aligned(rec, name)

    def records(self, key, n: int, device, direction=None):
        """The uint8 [n, record_bytes(direction)] record buffer of `key`; `direction` is required: the two directions
        may have different record widths. Keyed by shape too and never replaced, so a HIP graph captured around the
        kernels at one size keeps valid pointers after another size has run (CutCodec._buf)."""
        if direction is None:
            raise ValueError("MxCut.records: direction= is required ('fwd' or 'bwd')")
        width = self.record_bytes(direction)
        k = (key, int(n), width, str(torch.device(device)))
        t = self._bufs.get(k)
        if t is None:
            t = torch.empty((int(n), width), dtype=torch.uint8, device=device)
            self._bufs[k] = t
        return t

    def encode(self, x, rec, direction: str = "fwd", step=None, row0: int = 0):
        """x (bf16 [n, ...]) -> rec (uint8 [n, record_bytes(direction)]) in `direction`'s format."""
        fmt, n = CUTMX_FORMATS[self._name(direction)], Fp8Cut._rows(x, "x")
        self._records(rec, n, direction)
        _lib.call("slk_cutmx_encode", x.data_ptr(), n, fmt, rec.data_ptr(), _stream(x))
        return rec

    def decode(self, rec, out, err_flag, direction: str = "fwd"):
        """rec -> out (bf16 [n, ...]); a malformed header decodes its sample to NaNs, a scale byte below 27 its block,
        and either sets err_flag (int32 [1]); a poisoned block (scale byte 0xFF) decodes to 32 NaNs without the flag."""
        fmt, n = CUTMX_FORMATS[self._name(direction)], Fp8Cut._rows(out, "out")
        self._records(rec, n, direction)
        _dev(err_flag, "err_flag", (1,), torch.int32)
        _lib.call("slk_cutmx_decode", rec.data_ptr(), n, fmt, out.data_ptr(), err_flag.data_ptr(), _stream(out))
        return out

    def roundtrip(self, x, out, direction: str, step=None, row0: int = 0):
        """out = decode(encode(x)) bit for bit in one launch, no record in memory; out may be x."""
        fmt, n = CUTMX_FORMATS[self._name(direction)], Fp8Cut._rows(x, "x")
        if Fp8Cut._rows(out, "out") != n:
            raise ValueError(f"out: expected {n} samples like x, got {out.shape[0]}")
        _lib.call("slk_cutmx_roundtrip", x.data_ptr(), n, fmt, out.data_ptr(), _stream(x))
        return out


def check_cut_codec(codec):
    """A trainer's / hub's codec argument: an Fp8Cut, an MxCut or None."""
    if codec is not None and not isinstance(codec, (Fp8Cut, MxCut)):
        raise TypeError(f"expected splitcnn.codec.Fp8Cut, splitcnn.codec.MxCut or None, got {type(codec).__name__}")
    return codec
