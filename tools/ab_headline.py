#!/usr/bin/env python3
"""Interleaved A/B of the headline kernel (CookTorrance eval+pdf, 100 M pairs) between library builds loaded into
one process, with a bitwise comparison of their outputs.

    python tools/ab_headline.py parent=bbm_amd/lib_ab/parent/libbbm_hip.so new=bbm_amd/lib/libbbm_hip.so \
        [--rounds 6] [--steps 20] [--pairs 100000000] [--exact]

Each round times every arm once, in turn: 5 warm-up launches, 0.3 s of untimed launches (bench.py's settle rule),
then `steps` launches between two events.  Prints one line per (round, arm), then per arm the median and range,
then whether the arms' outputs (rgb, pdf of all pairs) are the same bits.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("arms", nargs="+", help="name=path/to/libbbm_hip.so")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--model", default="CookTorrance")
    ap.add_argument("--exact", action="store_true")
    args = ap.parse_args()
    import bbm_amd
    from bbm_amd import _lib
    n = args.pairs
    din = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=1)
    dout = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=1)
    params = bbm_amd.BsdfModel(args.model).parameter_values()
    pbuf = (ctypes.c_float * len(params))(*[float(p) for p in params])
    s = torch.cuda.current_stream().cuda_stream
    arms = []
    for spec in args.arms:
        name, path = spec.split("=", 1)
        lib = ctypes.CDLL(os.path.join(ROOT, path))
        for fn in ("bbm_hip_eval_pdf", "bbm_hip_model_id", "bbm_hip_set_exact_subnormals"):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.SIGNATURES[fn]
        lib.bbm_hip_set_exact_subnormals(1 if args.exact else 0)
        out = torch.empty((4, n), dtype=torch.float32, device="cuda")
        mid = lib.bbm_hip_model_id(args.model.encode())

        def launch(lib=lib, out=out, mid=mid):
            rc = lib.bbm_hip_eval_pdf(mid, pbuf, len(params), *[din[i].data_ptr() for i in range(3)],
                                      *[dout[i].data_ptr() for i in range(3)], None, n, 3, 0,
                                      *[out[i].data_ptr() for i in range(4)], s)
            assert rc == 0, rc
        arms.append((name, launch, out, []))
    for r in range(args.rounds):
        for name, launch, _, ms in arms:
            for _ in range(5):
                launch()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:
                for _ in range(10):
                    launch()
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
            print(f"r{r + 1} {name} {args.model}{' exact' if args.exact else ''} {ms[-1]:.4f} ms", flush=True)
    for name, _, _, ms in arms:
        print(f"# {name}: median {statistics.median(ms):.4f} ms, range {min(ms):.4f} .. {max(ms):.4f} "
              f"(spread {max(ms) - min(ms):.4f})")
    base = arms[0][2].view(torch.int32)
    for name, _, out, _ in arms[1:]:
        same = bool(torch.equal(base, out.view(torch.int32)))
        print(f"# outputs of {name} vs {arms[0][0]}: {'bit-identical' if same else 'DIFFERENT'} "
              f"({4 * n} floats)")
        assert same


if __name__ == "__main__":
    main()
