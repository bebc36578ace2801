"""Profiling only: fc1's backward of several libslk builds timed side by side in ONE process, interleaved rounds, HIP
events on one stream, real activations (as tools/x3_ab.py, whose --flush mechanism this uses).
Per library:  two  = slk_fc_wgrad then slk_fc_dgrad_amax back to back (the step's order before slk_fc_backward)
              one  = slk_fc_backward (libraries that have it)
              dgrad / wgrad = each of the two launches alone
After the timing every library's outputs are compared with torch.equal against the first library's `two`.
--flush reads 600 MB before every timed call, so every operand comes from HBM. --after-logits then runs the first
library's slk_fc_logits_xent (still outside the timing), so that pooled sits in the Infinity Cache as it does in the
step, where the logits launch has just read it.
usage: python tools/fc_backward_ab.py parent.so tree.so variant.so ... [--rounds 20] [--B 4096,512] [--flush]
       [--after-logits] [--cases two,one]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "split-learning-k8s_amd"), ROOT]

import torch  # noqa: E402


def run(args, B, dev, flushbuf, flushout):
    from splitcnn import ops
    from splitcnn.data import SyntheticMNIST, init_models
    from splitcnn.engine import ClientStage
    a, b = init_models(seed=1)
    x, y = SyntheticMNIST(2).batch(B)
    act = ClientStage(a, device=dev).forward(x.to(dev)).clone()
    W2, b2 = b.conv2.weight.detach().to(dev).contiguous(), b.conv2.bias.detach().to(dev).contiguous()
    W3, b3 = b.fc1.weight.detach().to(dev).contiguous(), b.fc1.bias.detach().to(dev).contiguous()
    pooled, _ = ops.conv2_fwd_pool(act, W2, b2)
    _, _, dl = ops.fc_logits_xent(pooled, W3, b3, y.to(dev), 1.0 / B)
    P = ctypes.c_void_p
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases, outs = {}, {}
    prior = None
    for path in args.libs:
        L = ctypes.CDLL(os.path.abspath(path), mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)  # own symbols first
        tag = os.path.basename(path).replace(".so", "")
        L.slk_build_id.restype = ctypes.c_char_p
        print(f"B={B} {tag}: build id {L.slk_build_id().decode()[:12]}", flush=True)
        for n in ("slk_fc_wgrad_nslab", "slk_fc_wgrad", "slk_fc_dgrad_amax"):
            getattr(L, n).restype = ctypes.c_int
        L.slk_fc_wgrad.argtypes = [P] * 3 + [ctypes.c_int, P]
        L.slk_fc_dgrad_amax.argtypes = [P] * 4 + [ctypes.c_int, P]
        new = lambda: [torch.full((B, 9216), float("nan"), device=dev), torch.full((B,), float("nan"), device=dev),  # noqa: E731
                       torch.full((L.slk_fc_wgrad_nslab(B), 92170), float("nan"), device=dev)]
        if args.after_logits and prior is None:
            L.slk_fc_logits_xent.restype = ctypes.c_int
            L.slk_fc_logits_xent.argtypes = [P] * 7 + [ctypes.c_float, P, ctypes.c_int, P]
            yl, lg, li, dl2 = y.to(dev), torch.empty(B, 10, device=dev), torch.empty(B, device=dev), torch.empty_like(dl)
            prior = (lambda L=L: L.slk_fc_logits_xent(p(pooled), p(W3), p(b3), p(yl), p(lg), p(li), p(dl2), 1.0 / B, None,
                                                      B, st))
        o2 = new()
        cases[f"two {tag}"] = (lambda L=L, o=o2: L.slk_fc_wgrad(p(dl), p(pooled), p(o[2]), B, st)
                               | L.slk_fc_dgrad_amax(p(dl), p(W3), p(o[0]), p(o[1]), B, st))
        cases[f"wgrad {tag}"] = (lambda L=L, o=o2: L.slk_fc_wgrad(p(dl), p(pooled), p(o[2]), B, st))
        cases[f"dgrad {tag}"] = (lambda L=L, o=o2: L.slk_fc_dgrad_amax(p(dl), p(W3), p(o[0]), p(o[1]), B, st))
        outs[f"two {tag}"] = o2
        if hasattr(L, "slk_fc_backward"):
            L.slk_fc_backward.restype = ctypes.c_int
            L.slk_fc_backward.argtypes = [P] * 6 + [ctypes.c_int, P]
            o1 = new()
            cases[f"one {tag}"] = (lambda L=L, o=o1: L.slk_fc_backward(p(dl), p(W3), p(pooled), p(o[0]), p(o[1]), p(o[2]),
                                                                       B, st))
            outs[f"one {tag}"] = o1
    cases = {k: f for k, f in cases.items() if k.split()[0] in args.cases.split(",")}
    outs = {k: o for k, o in outs.items() if k in cases}
    times = {k: [] for k in cases}
    for _ in range(3):
        for f in cases.values():
            assert f() == 0
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, f in cases.items():
            if flushbuf is not None:  # a READ of 600 MB evicts with clean lines: operands come from HBM, as in the step
                torch.sum(flushbuf, dim=0, out=flushout)
            if prior is not None:
                assert prior() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    for k, v in sorted(times.items()):
        v.sort()
        print(f"B={B} {k:28s} median {1e3 * v[len(v) // 2]:7.2f} us  min {1e3 * v[0]:7.2f}  q1 {1e3 * v[len(v) // 4]:7.2f}  "
              f"q3 {1e3 * v[(3 * len(v)) // 4]:7.2f}  max {1e3 * v[-1]:7.2f}", flush=True)
    ref = next(iter(outs.values()))
    for k, o in outs.items():
        same = all(torch.equal(u, v) for u, v in zip(o, ref))
        print(f"B={B} check {k:28s} dpooled, dp_amax, slabs torch.equal to the first library's two launches: {same}",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--B", default="4096,512")
    ap.add_argument("--cases", default="two,one,dgrad,wgrad")
    ap.add_argument("--after-logits", action="store_true",
                    help="run slk_fc_logits_xent before every timed call (outside the timing): pooled is in the "
                         "Infinity Cache, as in the step")
    ap.add_argument("--flush", action="store_true",
                    help="read 600 MB before every timed call (outside the timing): operands come from HBM, "
                         "not the 256 MB Infinity Cache, as inside the step")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flushbuf = torch.ones(150_000_000, device=dev) if args.flush else None
    flushout = torch.empty((), device=dev) if args.flush else None
    for B in (int(b) for b in args.B.split(",")):
        run(args, B, dev, flushbuf, flushout)


if __name__ == "__main__":
    main()
