"""Check only: the MX cut kernels' two conversions against each other on the GPU, bit for bit. The product library
converts e2m1 with gfx950's v_cvt_scalef32_pk_fp4_f32 / v_cvt_scalef32_pk_f32_fp4 (scale operand 1.0) and e4m3 with
v_cvt_pk_fp8_f32 / v_cvt_f32_fp8; a variant built with -DSLK_CUTMX_HWCVT=0 runs the integer arithmetic of
csrc/slk_cutmx.h (the form that compiles for the host and is held there to tests/cutmx_ref.py).

  tools/build_variant.sh cutmx_int "-DSLK_CUTMX_HWCVT=0" && python tools/cutmx_cvt_check.py build_abl/cutmx_int.so

Inputs, both formats: for every block exponent e in [-100, 126 | 120], blocks whose first element pins e (F_MAX * 2^e;
the largest finite bf16 for the top e) and whose other 31 elements run through EVERY bf16 value of both signs that can
meet that e (|x| * 2^-e <= F_MAX, down to the subnormals and both zeros) — encode, decode and roundtrip compared; and
every code, in either nibble for e2m1, under every scale byte 0..255 decoded (the error flag compared too). Prints one
JSON line with the count of differing bytes / elements per comparison and the first few differences; exits nonzero on
any difference."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from splitcnn import _lib  # noqa: E402
from splitcnn.codec import CUT8_SAMPLE, CUTMX_BLOCK, CUTMX_FORMATS, CUTMX_RECORD  # noqa: E402

P, I = ctypes.c_void_p, ctypes.c_int
HEADER, PAYLOAD = 16, 16 + CUT8_SAMPLE // CUTMX_BLOCK
FMAX = {"e2m1": 6.0, "e4m3": 448.0}
E_HI = {"e2m1": 126, "e4m3": 120}


def variant(path):
    lib = ctypes.CDLL(path)
    lib.slk_cutmx_encode.argtypes = [P, I, I, P, P]
    lib.slk_cutmx_decode.argtypes = [P, I, I, P, P, P]
    lib.slk_cutmx_roundtrip.argtypes = [P, I, I, P, P]
    return lib


def bf16_bits(v: float) -> int:
    return int(torch.tensor([v], dtype=torch.bfloat16).view(torch.int16).item()) & 0xffff


def samples(name):
    """uint16 [n, 16384]: the blocks described above, padded with zero blocks."""
    blocks = []
    for e in range(-100, E_HI[name] + 1):
        top = 0x7f7f if e == E_HI[name] else bf16_bits(FMAX[name] * 2.0 ** e)
        mag = np.arange(top + 1, dtype=np.uint16)
        vals = np.concatenate([mag, mag | 0x8000])
        vals = np.concatenate([vals, np.zeros(-len(vals) % 31, dtype=np.uint16)]).reshape(-1, 31)
        blocks.append(np.concatenate([np.full((len(vals), 1), top, dtype=np.uint16), vals], 1))
    flat = np.concatenate(blocks).reshape(-1)
    flat = np.concatenate([flat, np.zeros(-len(flat) % CUT8_SAMPLE, dtype=np.uint16)])
    return flat.reshape(-1, CUT8_SAMPLE)


def all_codes(name):
    """uint8 [n, R]: every code under every scale byte 0..255 (e2m1: each code in the low and in the high nibble)."""
    R = CUTMX_RECORD[name]
    if name == "e2m1":
        c = np.arange(16, dtype=np.uint8)
        block = np.concatenate([c[0::2] | (c[1::2] << 4), c[1::2] | (c[0::2] << 4)])   # 16 bytes = 32 codes
        per = 1
    else:
        block = np.arange(256, dtype=np.uint8)                                          # 8 blocks of 32 bytes
        per = 8
    nblocks = 256 * per
    n = nblocks * CUTMX_BLOCK // CUT8_SAMPLE + (1 if nblocks * CUTMX_BLOCK % CUT8_SAMPLE else 0)
    rec = np.zeros((n, R), dtype=np.uint8)
    head = rec[:, :HEADER].view(np.uint32)
    head[:, 0], head[:, 1] = CUTMX_BLOCK, 0x10 + CUTMX_FORMATS[name]
    scales = np.full(n * 512, 127, dtype=np.uint8)
    scales[:nblocks] = np.repeat(np.arange(256, dtype=np.uint8), per)
    rec[:, HEADER:PAYLOAD] = scales.reshape(n, 512)
    pay = np.zeros(n * (R - PAYLOAD), dtype=np.uint8)
    pay[:256 * len(block)] = np.tile(block, 256)
    rec[:, PAYLOAD:] = pay.reshape(n, R - PAYLOAD)
    return rec


def main():
    other = variant(sys.argv[1])
    own = _lib.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"tool": "cutmx_cvt_check", "differences": {}, "examples": {}}
    for name, fmt in CUTMX_FORMATS.items():
        bits = samples(name)
        n = bits.shape[0]
        out[f"{name}_samples"], out[f"{name}_elements"] = n, int(bits.size)
        x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(dev)
        allrec_host = all_codes(name)
        got = []
        for lib in (own, other):
            rec = torch.full((n, CUTMX_RECORD[name]), 0xA5, dtype=torch.uint8, device=dev)
            dec, rt = torch.zeros_like(x), torch.zeros_like(x)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            for rc in (lib.slk_cutmx_encode(x.data_ptr(), n, fmt, rec.data_ptr(), st),
                       lib.slk_cutmx_decode(rec.data_ptr(), n, fmt, dec.data_ptr(), err.data_ptr(), st),
                       lib.slk_cutmx_roundtrip(x.data_ptr(), n, fmt, rt.data_ptr(), st)):
                assert rc == 0, rc
            torch.cuda.synchronize()
            assert int(err.item()) == 0
            allrec = torch.from_numpy(allrec_host).to(dev)
            alldec = torch.zeros((allrec.shape[0], CUT8_SAMPLE), dtype=torch.bfloat16, device=dev)
            err2 = torch.zeros(1, dtype=torch.int32, device=dev)
            assert lib.slk_cutmx_decode(allrec.data_ptr(), allrec.shape[0], fmt, alldec.data_ptr(), err2.data_ptr(), st) == 0
            torch.cuda.synchronize()
            got.append({"encode": rec.cpu(), "decode": dec.view(torch.int16).cpu(), "roundtrip": rt.view(torch.int16).cpu(),
                        "decode_all_codes": alldec.view(torch.int16).cpu(), "decode_all_codes_flag": err2.cpu()})
        for k in got[0]:
            diff = got[0][k] != got[1][k]
            out["differences"][f"{name}_{k}"] = int(diff.sum())
            if diff.any():
                idx = diff.reshape(-1).nonzero().reshape(-1)[:8].tolist()
                a, b = got[0][k].reshape(-1), got[1][k].reshape(-1)
                out["examples"][f"{name}_{k}"] = [[i, int(a[i]) & 0xffff, int(b[i]) & 0xffff] for i in idx]
                if k in ("decode", "roundtrip"):   # the inputs of the first differences
                    out["examples"][f"{name}_{k}_inputs"] = [int(bits.reshape(-1)[i]) for i in idx]
        out[f"{name}_roundtrip_is_decode_of_encode"] = bool(torch.equal(got[0]["decode"], got[0]["roundtrip"]))
    print(json.dumps(out))
    sys.exit(1 if any(out["differences"].values()) else 0)


if __name__ == "__main__":
    main()
