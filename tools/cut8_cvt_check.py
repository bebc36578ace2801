"""Check only: the FP8 cut kernels' two conversions against each other on the GPU, bit for bit. The product library
converts with gfx950's v_cvt instructions; a variant built with -DSLK_CUT8_HWCVT=0 runs the integer arithmetic of
csrc/slk_cut8.h (the form that compiles for the host and was checked there against torch's float8 casts).

  tools/build_variant.sh cut8_int "-DSLK_CUT8_HWCVT=0" && python tools/cut8_cvt_check.py build_abl/cut8_int.so

Inputs, both formats: for every amax exponent field 1..254 with mantissa 0x00 / 0x60 / 0x61 / 0x7f, and for subnormal
amax values, one sample holding EVERY bf16 value of both signs within 36 binades below amax (further down everything
converts to zero in either format) — encode, decode and roundtrip compared; and every one of the 256 codes decoded
under every exponent in [-100, 127]. Prints one JSON line; exits nonzero on any difference."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]
from splitcnn import _lib  # noqa: E402
from splitcnn.codec import CUT8_RECORD, CUT8_SAMPLE  # noqa: E402

P, I = ctypes.c_void_p, ctypes.c_int


def variant(path):
    lib = ctypes.CDLL(path)
    lib.slk_cut8_encode.argtypes = [P, I, I, P, P]
    lib.slk_cut8_decode.argtypes = [P, I, I, P, P, P]
    lib.slk_cut8_roundtrip.argtypes = [P, I, I, P, P]
    return lib


def samples():
    rows = []
    amax = [(ex << 7) | man for ex in range(1, 255) for man in (0x00, 0x60, 0x61, 0x7f)] + [0x01, 0x55, 0x7f]
    for a in amax:
        mag = np.arange(max(0, a - 36 * 128), a + 1, dtype=np.uint16)
        row = np.zeros(CUT8_SAMPLE, dtype=np.uint16)
        row[:len(mag)] = mag
        row[len(mag):2 * len(mag)] = mag | 0x8000
        rows.append(row)
    return np.stack(rows)


def main():
    other = variant(sys.argv[1])
    own = _lib.load()
    dev = torch.device("cuda:0")
    bits = samples()
    n = bits.shape[0]
    x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"tool": "cut8_cvt_check", "samples": n, "elements": int(bits.size), "differences": {}}
    for fmt in (0, 1):
        got = []
        for lib in (own, other):
            rec = torch.full((n, CUT8_RECORD), 0xFF, dtype=torch.uint8, device=dev)
            dec, rt = torch.zeros_like(x), torch.zeros_like(x)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            for rc in (lib.slk_cut8_encode(x.data_ptr(), n, fmt, rec.data_ptr(), st),
                       lib.slk_cut8_decode(rec.data_ptr(), n, fmt, dec.data_ptr(), err.data_ptr(), st),
                       lib.slk_cut8_roundtrip(x.data_ptr(), n, fmt, rt.data_ptr(), st)):
                assert rc == 0, rc
            # every code under every exponent
            allrec = torch.zeros((228, CUT8_RECORD), dtype=torch.uint8)
            head = allrec[:, :16].numpy().view(np.int32)
            head[:, 0] = np.arange(-100, 128)
            head[:, 1] = fmt
            allrec[:, 16:] = torch.arange(CUT8_SAMPLE).to(torch.uint8)
            allrec = allrec.to(dev)
            alldec = torch.zeros((228, CUT8_SAMPLE), dtype=torch.bfloat16, device=dev)
            assert lib.slk_cut8_decode(allrec.data_ptr(), 228, fmt, alldec.data_ptr(), err.data_ptr(), st) == 0
            torch.cuda.synchronize()
            assert int(err.item()) == 0
            got.append({"encode": rec.cpu(), "decode": dec.view(torch.int16).cpu(), "roundtrip": rt.view(torch.int16).cpu(),
                        "decode_all_codes": alldec.view(torch.int16).cpu()})
        for k in got[0]:
            out["differences"][f"fmt{fmt}_{k}"] = int((got[0][k] != got[1][k]).sum())
        assert torch.equal(got[0]["decode"], got[0]["roundtrip"])
    print(json.dumps(out))
    sys.exit(1 if any(out["differences"].values()) else 0)


if __name__ == "__main__":
    main()
