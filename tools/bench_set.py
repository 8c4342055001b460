"""Material sets against what a caller writes without them: ms per call over a batch whose
lanes belong to four tables of different models.

  python tools/bench_set.py [--lanes 100000000] [--reps 25] [--warmup 5]

Four tables of 16 materials each (CookTorrance, GGX, Aggregate<Lambertian,CookTorrance>, Lambertian), global ids
(i) uniformly random and (ii) already grouped by table; world eval_pdf with the cosine and world sample_eval with the
weight alone.  Variants, interleaved launch by launch:
  (a) floor     one table call over all lanes of CookTorrance alone;
  (b) torch     the same result without sets: torch.argsort(rows, stable=True), indexed gathers, the per-table calls on
                slices, indexed writes back;
  (c) set       the set call with material= (a fresh plan per call);
  (d) set+plan  the set call on a plan made once.
Inputs stay resident in 16-byte aligned buffers; HIP events on the launch stream; the median (min-max) of --reps calls.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from tools.bench_varying import time_variants  # noqa: E402

ROWS = ["CookTorrance", "GGX", "Aggregate<Lambertian,CookTorrance>", "Lambertian"]
PER_TABLE = 16


def table_of(name):
    m = bbm_amd.BsdfModel(name)
    base = m.parameter_values()
    scale = np.linspace(0.7, 1.0, PER_TABLE, dtype=np.float32)[:, None]
    params = np.clip(base[None] * scale, m.parameter_lower_bound(), m.parameter_upper_bound()).astype(np.float32)
    return bbm_amd.MaterialTable(name, params)


def torch_pipeline(tables, offsets, ids, streams, call, outputs):
    """Variant (b).  streams: the (k, n) inputs; call(table, slices, local) -> the outputs of one table on its slice;
    outputs: preallocated result tensors, written back by index."""
    off = torch.tensor(offsets[1:-1], dtype=torch.int32, device="cuda")
    first = torch.tensor(offsets[:-1], dtype=torch.int32, device="cuda")
    rows = torch.bucketize(ids, off, right=True)
    order = torch.argsort(rows, stable=True)
    bounds = [0] + torch.cumsum(torch.bincount(rows, minlength=len(tables)), 0).tolist()
    local = (ids - first[rows])[order]
    sorted_in = [x[..., order] for x in streams]
    for k, t in enumerate(tables):
        a, b = bounds[k], bounds[k + 1]
        if a == b:
            continue
        res = call(t, [x[..., a:b] for x in sorted_in], local[a:b])
        for dst, r in zip(outputs, res):
            dst[..., order[a:b]] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    n = a.lanes
    assert n % 4 == 0, "--lanes: a multiple of four keeps every row of the (k, n) buffers 16-byte aligned"
    tables = [table_of(name) for name in ROWS]
    mset = bbm_amd.MaterialSet(tables)
    total = len(mset)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rnd = torch.randint(0, total, (n,), dtype=torch.int32, device="cuda", generator=g)
    id_orders = {"random": rnd, "grouped": torch.sort(rnd).values.contiguous()}
    floor_ids = (rnd % PER_TABLE).contiguous()
    din = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=1)
    dout = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=1)
    normal = bbm_amd.fill_directions(0xBB5EED, 2, 0, n, mode=1)
    xi = torch.rand((2, n), dtype=torch.float32, device="cuda", generator=g)
    rows3 = lambda x: tuple(x[k] for k in range(x.shape[0]))

    def nee_table(t, s, local):
        rgb, pdf, cos = t.eval_pdf(rows3(s[1]), rows3(s[2]), material=local, normal=s[0], cosine=True)
        return rgb, pdf, cos

    def bounce_table(t, s, local):
        smp, _, w = t.sample_eval(rows3(s[1]), rows3(s[2]), material=local, normal=s[0], value=False)
        return smp.direction, smp.pdf, smp.flag, w
    nee_out = [torch.empty((3, n), device="cuda"), torch.empty((n,), device="cuda"), torch.empty((n,), device="cuda")]
    bounce_out = [torch.empty((3, n), device="cuda"), torch.empty((n,), device="cuda"),
                  torch.empty((n,), dtype=torch.int32, device="cuda"), torch.empty((3, n), device="cuda")]
    cases = {
        "world eval_pdf + cosine": dict(
            floor=lambda: tables[0].eval_pdf(din, dout, material=floor_ids, normal=normal, cosine=True),
            torch=lambda ids: torch_pipeline(tables, mset.offsets, ids, [normal, din, dout], nee_table, nee_out),
            set=lambda **kw: mset.eval_pdf(din, dout, normal=normal, cosine=True, **kw)),
        "world sample_eval, weight": dict(
            floor=lambda: tables[0].sample_eval(dout, xi, material=floor_ids, normal=normal, value=False),
            torch=lambda ids: torch_pipeline(tables, mset.offsets, ids, [normal, dout, xi], bounce_table, bounce_out),
            set=lambda **kw: mset.sample_eval(dout, xi, normal=normal, value=False, **kw)),
    }
    for case, f in cases.items():
        for how, ids in id_orders.items():
            plan = mset.plan(ids)
            variants = {"(a) floor": f["floor"], "(b) torch": lambda: f["torch"](ids),
                        "(c) set": lambda: f["set"](material=ids), "(d) set+plan": lambda: f["set"](plan=plan)}
            times = time_variants(variants, a.reps, a.warmup)
            med = {k: statistics.median(t) for k, t in times.items()}
            spread = max(times["(b) torch"]) - min(times["(b) torch"])
            for k, t in times.items():
                print(json.dumps({"case": case, "ids": how, "lanes": n, "variant": k, "reps": len(t),
                                  "ms_median": round(med[k], 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                                  "vs_floor": round(med[k] / med["(a) floor"], 3)}), flush=True)
            print(json.dumps({"case": case, "ids": how, "torch_spread_ms": round(spread, 3),
                              "set_beats_torch_by_ms": round(med["(b) torch"] - med["(c) set"], 3),
                              "set_plan_beats_torch_by_ms": round(med["(b) torch"] - med["(d) set+plan"], 3),
                              "claim_holds": bool(med["(b) torch"] - med["(c) set"] > spread and
                                                  med["(b) torch"] - med["(d) set+plan"] > spread)}), flush=True)
            plan.close()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
