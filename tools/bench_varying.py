"""Per-lane parameters against the uniform kernels: ms per launch and algorithmic TB/s.

  python tools/bench_varying.py [--pairs 100000000] [--ribardiere-pairs 10000000] [--reps 25] [--warmup 5]

CookTorrance eval_pdf in three variants -- the uniform kernel (40 B / pair), `roughness` varying (44 B / pair), all five
parameters varying (60 B / pair) -- and Ribardiere uniform (its Student-T constructor once per thread under the capped
grid) against all six varying (the constructor once per pair).  Inputs and outputs stay resident; each variant is
timed with HIP events on the launch stream, the variants of a model interleaved launch by launch after a warm-up, and
the median over --reps launches is reported.  The byte counts are the arrays the call reads and writes once.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402


def ramp(lo, hi, n):
    return torch.linspace(lo, hi, n, dtype=torch.float32, device="cuda")


def time_variants(variants, reps, warmup):
    """variants: {label: callable}; -> {label: [ms per launch]}, interleaved."""
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return times


def report(model, n, variants, bytes_per_pair, reps, warmup):
    times = time_variants(variants, reps, warmup)
    base = None
    out = []
    for k, t in times.items():
        med = statistics.median(t)
        base = med if base is None else base
        row = {"model": model, "pairs": n, "variant": k, "bytes_per_pair": bytes_per_pair[k], "reps": len(t),
               "ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
               "tb_per_s": round(bytes_per_pair[k] * n / (med * 1e-3) / 1e12, 3), "vs_uniform": round(med / base, 3)}
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--ribardiere-pairs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)

    n = a.pairs
    din = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=0)
    dout = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=0)
    rgb = torch.empty((3, n), dtype=torch.float32, device="cuda")
    pdf = torch.empty((n,), dtype=torch.float32, device="cuda")
    m = bbm_amd.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5)
    rough = ramp(0.05, 0.6, n)
    rows = {"albedo": torch.stack([ramp(0.1, 0.9, n), ramp(0.9, 0.1, n), ramp(0.2, 0.7, n)]), "roughness": rough,
            "eta": ramp(1.2, 2.0, n)}
    report("CookTorrance", n, {
        "uniform": lambda: m.eval_pdf(din, dout, rgb=rgb, pdf=pdf),
        "roughness varying": lambda: m.eval_pdf(din, dout, rgb=rgb, pdf=pdf, varying={"roughness": rough}),
        "all 5 varying": lambda: m.eval_pdf(din, dout, rgb=rgb, pdf=pdf, varying=rows),
    }, {"uniform": 40, "roughness varying": 44, "all 5 varying": 60}, a.reps, a.warmup)
    del rows, rough

    k = a.ribardiere_pairs
    din, dout, rgb, pdf = din[:, :k].contiguous(), dout[:, :k].contiguous(), rgb[:, :k].contiguous(), pdf[:k].contiguous()
    r = bbm_amd.Ribardiere(albedo=[0.3, 0.5, 0.7], roughness=0.2, gamma=2.5, eta=1.5)
    rrows = {"albedo": torch.stack([ramp(0.1, 0.9, k), ramp(0.9, 0.1, k), ramp(0.2, 0.7, k)]),
             "roughness": ramp(0.05, 0.6, k), "gamma": ramp(1.6, 8.0, k), "eta": ramp(1.2, 2.0, k)}
    report("Ribardiere", k, {
        "uniform": lambda: r.eval_pdf(din, dout, rgb=rgb, pdf=pdf),
        "all 6 varying": lambda: r.eval_pdf(din, dout, rgb=rgb, pdf=pdf, varying=rrows),
    }, {"uniform": 40, "all 6 varying": 64}, a.reps, a.warmup)


if __name__ == "__main__":
    main()
