"""Material tables against the uniform and the per-lane-parameter kernels: ms per launch and algorithmic TB/s
(DESIGN.md section 4.15).

  python tools/bench_table.py [--pairs 100000000] [--bagher-pairs 10000000] [--reps 25] [--warmup 5]

CookTorrance eval_pdf: the uniform kernel (40 B / pair), the table path (44 B / pair: a 4-byte index more) with
M = 1, 16, 1 024 and 65 536 materials, each with random indices and with the same indices sorted (runs far longer than
a wave), and all five parameters varying (60 B / pair) at the parameters of the 1 024-material random case.
Aggregate<Lambertian,Bagher> eval_pdf: uniform, a 100-material table with random and sorted indices, and all 33
parameters varying (172 B / pair).  Inputs and outputs stay resident; each variant is timed with HIP events on the
launch stream, the variants of a model interleaved launch by launch after a warm-up, and the median and the range
over --reps launches are reported.  The byte counts are the arrays the call reads and writes once; a table's own
bytes are not counted (they are read through the caches, once per material at best).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from tools.bench_varying import report  # noqa: E402


def cooktorrance_ramp(m):
    t = np.linspace(0.0, 1.0, m, dtype=np.float32)
    return np.stack([0.2 + 0.6 * t, 0.8 - 0.5 * t, 0.3 + 0.3 * t, 0.05 + 0.55 * t, 1.3 + 0.4 * t], 1).astype(np.float32)


def indices(m, n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rnd = torch.randint(0, m, (n,), dtype=torch.int32, device="cuda", generator=g)
    return rnd, torch.sort(rnd).values.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000_000)
    ap.add_argument("--bagher-pairs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    torch.cuda.set_device(0)
    print('{"device": "%s"}' % torch.cuda.get_device_name(0), flush=True)

    n = a.pairs
    din = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=0)
    dout = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=0)
    rgb = torch.empty((3, n), dtype=torch.float32, device="cuda")
    pdf = torch.empty((n,), dtype=torch.float32, device="cuda")
    m = bbm_amd.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5)
    variants = {"uniform": lambda: m.eval_pdf(din, dout, rgb=rgb, pdf=pdf)}
    nbytes = {"uniform": 40}
    keep = []
    for count in (1, 16, 1024, 65536):
        params = cooktorrance_ramp(count) if count > 1 else m.parameter_values()[None]
        table = bbm_amd.MaterialTable("CookTorrance", params)
        rnd, srt = indices(count, n, count)
        keep.append((table, rnd, srt))
        for label, idx in (("random", rnd), ("sorted", srt)):
            if count == 1 and label == "sorted":
                continue
            key = f"table M={count} {label}"
            variants[key] = (lambda t=table, i=idx: t.eval_pdf(din, dout, rgb=rgb, pdf=pdf, material=i))
            nbytes[key] = 44
        if count == 1024:
            rows = torch.from_numpy(params).cuda()[rnd.long()].T.contiguous()
            vary = {"albedo": rows[0:3], "roughness": rows[3], "eta": rows[4]}
            variants["all 5 varying"] = lambda: m.eval_pdf(din, dout, rgb=rgb, pdf=pdf, varying=vary)
            nbytes["all 5 varying"] = 60
    report("CookTorrance", n, variants, nbytes, a.reps, a.warmup)
    del variants, keep, rows, vary

    k = a.bagher_pairs
    din, dout, rgb, pdf = din[:, :k].contiguous(), dout[:, :k].contiguous(), rgb[:, :k].contiguous(), pdf[:k].contiguous()
    name = "Aggregate<Lambertian,Bagher>"
    b = bbm_amd.BsdfModel(name)
    base = b.parameter_values()
    scale = np.linspace(0.8, 1.0, 100, dtype=np.float32)[:, None]
    params = np.clip(base[None] * scale, b.parameter_lower_bound(), b.parameter_upper_bound()).astype(np.float32)
    table = bbm_amd.MaterialTable(name, params)
    rnd, srt = indices(100, k, 100)
    rows = torch.from_numpy(params).cuda()[rnd.long()].T.contiguous()
    vary = {j: rows[j] for j in range(rows.shape[0])}
    report(name, k, {
        "uniform": lambda: b.eval_pdf(din, dout, rgb=rgb, pdf=pdf),
        "table M=100 random": lambda: table.eval_pdf(din, dout, rgb=rgb, pdf=pdf, material=rnd),
        "table M=100 sorted": lambda: table.eval_pdf(din, dout, rgb=rgb, pdf=pdf, material=srt),
        "all 33 varying": lambda: b.eval_pdf(din, dout, rgb=rgb, pdf=pdf, varying=vary),
    }, {"uniform": 40, "table M=100 random": 44, "table M=100 sorted": 44, "all 33 varying": 172}, a.reps, a.warmup)


if __name__ == "__main__":
    main()
