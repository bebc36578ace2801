"""Check only: the stochastic-rounding FP8 cut kernels (slk_cut8_encode_sr / slk_cut8_roundtrip_sr) on the GPU.

  python tools/cut8_sr_check.py --build-probe          # no GPU needed: build_abl/cut8_sr_probe.so
  tools/build_variant.sh cut8_int "-DSLK_CUT8_HWCVT=0" && python tools/cut8_sr_check.py build_abl/cut8_int.so
  (--probe=PATH: the probe library elsewhere; --probe-only: part 2 alone)

1. The two builds against each other, bit for bit: the product library and a -DSLK_CUT8_HWCVT=0 variant (the integer
   arithmetic of csrc/slk_cut8.h throughout) over tools/cut8_cvt_check.py's samples — every bf16 value of both signs
   within 36 binades below every amax exponent, plus four samples that span bf16's whole range below their amax — both formats, encode_sr and roundtrip_sr, several (seed, step, row0);
   the records are also decoded by slk_cut8_decode and compared with roundtrip_sr.
2. The bare instructions v_cvt_sr_fp8_f32 / v_cvt_sr_bf8_f32 (tools/cut8_sr_probe.hip) on chosen (y, r): y = sig * 2^q
   with an integer sig < 256 covering every s = 1..40 of the rule (include/slk.h, "stochastic rounding") in each format's
   subnormal range, results below the smallest subnormal, the normal range and the carry into the next binade. Each y is
   converted with random and threshold-edge random words and compared with three candidate mappings of r to `up`
   ("low": the low nb = 23 - M bits of r added to the discarded bits; "high": the same with r's top nb bits; "natural":
   r < T on 32 bits), and its round-ups are counted over 2^22 consecutive words and over 2^22 words spaced 2^10 apart
   (every pattern of r's top 22 bits), against rem * 2^(22 - s) and against the law at nb bits (exact for s <= nb,
   floor(rem * 2^(nb - s)) above, each pattern of the nb bits met 2^(22 - nb) times).
Prints one JSON line (stored as profiles/cut8_sr_check.txt); exits nonzero on a difference between the builds."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT, os.path.join(ROOT, "tools")]
PROBE_SRC = os.path.join(ROOT, "tools", "cut8_sr_probe.hip")
PROBE_LIB = os.path.join(ROOT, "build_abl", "cut8_sr_probe.so")
P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
FMT = {0: (3, -6), 1: (2, -14)}   # fmt word -> (M, EMIN)
KEYS = [(0, 0, 0), (5, 1, 0), (0xDEADBEEF, 0x80000003, 7), (1, 12345, 4091)]   # (seed, step, row0)


def build_probe():
    from splitcnn.build import ARCH, _hipcc
    os.makedirs(os.path.dirname(PROBE_LIB), exist_ok=True)
    subprocess.run([_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", PROBE_SRC, "-o", PROBE_LIB],
                   check=True)
    return PROBE_LIB


# ------------------------------------------------------------------------------------------ the bare instruction
def split(sig, q, fmt):
    """(s, k, rem, lo code) of y = sig * 2^q as the rule derives them (s > 0 here)."""
    M, EMIN = FMT[fmt]
    p = sig.bit_length() - 1 + q
    pe = max(p, EMIN)
    s = pe - M - q
    k = sig >> s
    return s, k, sig - (k << s), k + ((pe - EMIN) << M)


def up_model(model, rem, s, r, nb):
    if model == "natural":
        return int(r < (rem << (32 - s) if s <= 32 else rem >> (s - 32)))
    T = rem << (nb - s) if s <= nb else rem >> (s - nb)
    bits = (r & ((1 << nb) - 1)) if model == "low" else (r >> (32 - nb))
    return (bits + T) >> nb


def probe_inputs(fmt):
    """[(sig, q)] with s >= 1: the subnormal range at every s = 1..40, the normal range, the top of a binade."""
    M, EMIN = FMT[fmt]
    out = []
    for s in range(1, 41):
        q = EMIN - M - s
        sigs = {1, 3, 5, 0x55, 0x80, 0x81, 0xAA, 0xC0, 0xFF, (1 << min(s, 8)) - 1, 1 << min(s - 1, 7), (1 << min(s - 1, 7)) + 1}
        for sig in sorted(sigs):
            if 0 < sig < 256 and sig.bit_length() - 1 <= M + s:   # p <= EMIN: the quantum is the subnormal one
                out.append((sig, q))
    for h in range(M + 1, 8):                                      # normal range: s = h - M
        for sig in {1 << h, (1 << h) + 1, (1 << (h + 1)) - 1, (0xAA >> (7 - h)) | (1 << h), (0xD5 >> (7 - h)) | 1}:
            if sig.bit_length() - 1 == h:
                for p in (EMIN + 1, 0, 5):
                    out.append((sig, p - h))
    return sorted(set(out))


def probe(dev):
    import torch
    lib = ctypes.CDLL(PROBE_LIB)
    lib.probe_pairs.argtypes = [P, P, I, I, P, P]
    lib.probe_count.argtypes = [P, P, I, I, I, I, P, P]
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(7)
    res = {}
    for fmt, name in ((0, "e4m3"), (1, "e5m2")):
        M, _ = FMT[fmt]
        nb = 23 - M
        ys = probe_inputs(fmt)
        cases = [(sig, q) + split(sig, q, fmt) for sig, q in ys]
        assert {c[2] for c in cases} >= set(range(1, 41))
        # pairs: 48 random words and the threshold edges of each model, with random other bits
        py, pr, meta = [], [], []
        for ci, (sig, q, s, k, rem, lo) in enumerate(cases):
            words = [int(w) for w in rng.integers(0, 1 << 32, 48, dtype=np.uint64)] + [0, 0xFFFFFFFF]
            T = rem << (nb - s) if s <= nb else rem >> (s - nb)
            for edge in ((1 << nb) - T - 1, (1 << nb) - T):
                if 0 <= edge < (1 << nb):
                    hi = int(rng.integers(0, 1 << (32 - nb)))
                    words += [edge | (hi << nb), (edge << (32 - nb)) | int(rng.integers(0, 1 << (32 - nb)))]
            T32 = rem << (32 - s) if s <= 32 else rem >> (s - 32)
            words += [w for w in (T32 - 1, T32) if 0 <= w < (1 << 32)]
            for w in words:
                for sign in (1.0, -1.0):
                    py.append(sign * sig * 2.0 ** q)
                    pr.append(w)
                    meta.append((ci, sign < 0))
        y = torch.tensor(py, dtype=torch.float32, device=dev)
        assert np.array_equal(y.cpu().double().numpy(), np.array(py))
        r = torch.from_numpy(np.array(pr, dtype=np.uint32).view(np.int32)).to(dev)
        code = torch.zeros(len(py), dtype=torch.uint8, device=dev)
        assert lib.probe_pairs(y.data_ptr(), r.data_ptr(), len(py), fmt, code.data_ptr(), st) == 0
        code = code.cpu().numpy()
        miss = {"low": 0, "high": 0, "natural": 0}
        neighbours = 0
        for (ci, neg), w, c in zip(meta, pr, code):
            _, _, s, _, rem, lo = cases[ci]
            neighbours += int((c & 0x7f) in (lo, lo + 1) and bool(c & 0x80) == neg)
            for m in miss:
                miss[m] += int(c != ((lo + up_model(m, rem, s, w, nb)) | (0x80 if neg else 0)))
        # counts: 2^22 words from 0, and 2^22 words 2^10 apart
        cy = torch.tensor([sig * 2.0 ** q for sig, q, *_ in cases], dtype=torch.float32, device=dev)
        lo = torch.tensor([c[5] for c in cases], dtype=torch.uint8, device=dev)
        counts = {}
        for label, shift in (("consecutive", 0), ("spaced_1024", 10)):
            cnt = torch.zeros(len(cases), dtype=torch.int32, device=dev)
            assert lib.probe_count(cy.data_ptr(), lo.data_ptr(), len(cases), fmt, 22, shift, cnt.data_ptr(), st) == 0
            got = cnt.cpu().numpy().astype(np.int64)
            law = np.array([(rem << (22 - s)) if s <= 22 else (rem >> (s - 22)) for _, _, s, _, rem, _ in cases])
            # the law at nb bits, each pattern of them met 2^(22 - nb) times: exact for s <= nb, floored above
            at_nb = np.array([((rem << (nb - s)) if s <= nb else (rem >> (s - nb))) << (22 - nb) for _, _, s, _, rem, _ in cases])
            bad = sorted({cases[i][2] for i in np.nonzero(got != law)[0]})
            counts[label] = {"cases": len(cases), "equal_to_rem_times_2^(22-s)": int((got == law).sum()),
                             "s_with_a_difference": bad,
                             "equal_to_the_law_at_nb_bits": int((got == at_nb).sum()),
                             "rem0_rounds_up": int(sum(g for g, c in zip(got, cases) if c[4] == 0))}
        res[name] = {"nb_candidate": nb, "y_values": len(cases), "s_covered": [1, 40], "pairs": len(py),
                     "pairs_on_a_neighbouring_code_with_x_sign": neighbours, "pair_mismatches_by_mapping": miss,
                     "round_up_counts_over_2^22_words": counts}
    return res


# ------------------------------------------------------------------------------------------ the two builds
def variant(path):
    lib = ctypes.CDLL(path)
    lib.slk_cut8_encode_sr.argtypes = [P, I, I, P, U, P, I, P]
    lib.slk_cut8_roundtrip_sr.argtypes = [P, I, I, P, U, P, I, P]
    lib.slk_cut8_decode.argtypes = [P, I, I, P, P, P]
    return lib


def builds(dev, other_path):
    import torch
    from cut8_cvt_check import samples
    from splitcnn import _lib
    from splitcnn.codec import CUT8_RECORD, CUT8_SAMPLE
    own, other = _lib.load(), variant(other_path)
    # ... plus samples that reach down to the bottom of bf16's range: every fourth magnitude up to amax, both signs
    # (products x * 2^-e below float32's normal range included)
    wide = []
    for a in (0x7f7f, 0x4000, 0x3000, 0x0c00):
        mag = np.arange(0, a + 1, 4, dtype=np.uint16)
        row = np.zeros(CUT8_SAMPLE, dtype=np.uint16)
        row[:len(mag)] = mag
        row[len(mag):2 * len(mag)] = mag | 0x8000
        row[-1] = a
        wide.append(row)
    bits = np.concatenate([samples(), np.stack(wide)])
    n = bits.shape[0]
    x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {"samples": n, "elements": int(bits.size), "keys_seed_step_row0": KEYS, "differences": {}}
    for fmt in (0, 1):
        for seed, step, row0 in KEYS:
            ctr = torch.from_numpy(np.array([step], dtype=np.uint32).view(np.int32)).to(dev)
            got = []
            for lib in (own, other):
                rec = torch.full((n, CUT8_RECORD), 0xFF, dtype=torch.uint8, device=dev)
                dec, rt = torch.zeros_like(x), torch.zeros_like(x)
                err = torch.zeros(1, dtype=torch.int32, device=dev)
                for rc in (lib.slk_cut8_encode_sr(x.data_ptr(), n, fmt, rec.data_ptr(), seed, ctr.data_ptr(), row0, st),
                           lib.slk_cut8_decode(rec.data_ptr(), n, fmt, dec.data_ptr(), err.data_ptr(), st),
                           lib.slk_cut8_roundtrip_sr(x.data_ptr(), n, fmt, rt.data_ptr(), seed, ctr.data_ptr(), row0, st)):
                    assert rc == 0, rc
                torch.cuda.synchronize()
                assert int(err.item()) == 0
                got.append({"encode_sr": rec.cpu(), "roundtrip_sr": rt.view(torch.int16).cpu()})
                assert torch.equal(dec.view(torch.int16).cpu(), got[-1]["roundtrip_sr"])
            for k in got[0]:
                key = f"fmt{fmt}_{k}"
                out["differences"][key] = out["differences"].get(key, 0) + int((got[0][k] != got[1][k]).sum())
    return out


def main():
    if "--build-probe" in sys.argv:
        print(build_probe())
        return
    import torch
    global PROBE_LIB
    for a in sys.argv[1:]:
        if a.startswith("--probe="):
            PROBE_LIB = os.path.abspath(a.split("=", 1)[1])
    dev = torch.device("cuda:0")
    out = {"tool": "cut8_sr_check"}
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--probe-only" not in sys.argv:
        out["builds"] = builds(dev, paths[0])
    out["instruction"] = probe(dev)
    print(json.dumps(out))
    sys.exit(1 if any(out.get("builds", {}).get("differences", {}).values()) else 0)


if __name__ == "__main__":
    main()
