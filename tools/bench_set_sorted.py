"""Material sets in plan order against the lane-order set calls: ms per renderer bounce over
a batch whose lanes belong to four tables of different models.

  python tools/bench_set_sorted.py [--lanes 100000000] [--reps 25] [--warmup 5]

The set of tools/bench_set.py (four tables of 16 materials: CookTorrance, GGX, Aggregate<Lambertian,CookTorrance>,
Lambertian), global ids (i) uniformly random and (ii) already grouped by table.  One bounce is the world eval_pdf with
the cosine plus the world sample_eval with the weight alone.  Variants, interleaved launch by launch:
  (d2)    the two lane-order calls on a plan made once;
  (g)     plan.gather of the union of their inputs: normal, in, out and xi, 11 streams;
  (e)     the two calls with order="plan" on streams gathered once;
  (g)+(e) both;
  (t)     the per-row table calls issued by hand on the same slices, which is what (e) launches.
Then the gather alone in its two kernel shapes (bbm_hip_set_gather_shape 0 and 1), interleaved.
Inputs stay resident in 16-byte aligned buffers; HIP events on the launch stream; the median (min-max) of --reps calls.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from tools.bench_set import table_of, ROWS  # noqa: E402
from tools.bench_varying import time_variants  # noqa: E402


def rows_of(mset, plan, ids):
    """The per-row table calls of one bounce on the plan's slices: [(table, first slot, one past the last, local)]."""
    order = plan.order().long()
    first = torch.tensor(mset.offsets[:-1], dtype=torch.int32, device="cuda")
    out = []
    for k, t in enumerate(mset.tables):
        a, b = plan.segments[k], plan.segments[k + 1]
        if a == b:
            continue
        o = order[a:b]
        local = torch.where(o >= 0, ids[o.clamp(min=0)] - first[k], torch.full_like(o, -1, dtype=torch.int32))
        out.append((t, a, b, local.to(torch.int32).contiguous()))
    return out


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
    lib = bbm_amd._lib.load()
    tables = [table_of(name) for name in ROWS]
    mset = bbm_amd.MaterialSet(tables)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rnd = torch.randint(0, len(mset), (n,), dtype=torch.int32, device="cuda", generator=g)
    id_orders = {"random": rnd, "grouped": torch.sort(rnd).values.contiguous()}
    din = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=1)
    dout = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=1)
    normal = bbm_amd.fill_directions(0xBB5EED, 2, 0, n, mode=1)
    xi = torch.rand((2, n), dtype=torch.float32, device="cuda", generator=g)
    for how, ids in id_orders.items():
        plan = mset.plan(ids)
        s_normal, s_in, s_out, s_xi = plan.gather(normal, din, dout, xi)
        slices = rows_of(mset, plan, ids)

        def lane_order():
            mset.eval_pdf(din, dout, plan=plan, normal=normal, cosine=True)
            mset.sample_eval(dout, xi, plan=plan, normal=normal, value=False)

        def gather():
            plan.gather(normal, din, dout, xi)

        def plan_order():
            mset.eval_pdf(s_in, s_out, plan=plan, order="plan", normal=s_normal, cosine=True)
            mset.sample_eval(s_out, s_xi, plan=plan, order="plan", normal=s_normal, value=False)

        def both():
            gather()
            plan_order()

        def by_hand():
            for t, lo, hi, local in slices:
                t.eval_pdf(s_in[:, lo:hi], s_out[:, lo:hi], material=local, normal=s_normal[:, lo:hi], cosine=True)
            for t, lo, hi, local in slices:
                t.sample_eval(s_out[:, lo:hi], s_xi[:, lo:hi], material=local, normal=s_normal[:, lo:hi], value=False)
        variants = {"(d2) lane order": lane_order, "(g) gather": gather, "(e) plan order": plan_order,
                    "(g)+(e)": both, "(t) table calls by hand": by_hand}
        times = time_variants(variants, a.reps, a.warmup)
        med = {k: statistics.median(t) for k, t in times.items()}
        spread = {k: max(t) - min(t) for k, t in times.items()}
        for k, t in times.items():
            print(json.dumps({"ids": how, "lanes": n, "variant": k, "reps": len(t), "ms_median": round(med[k], 3),
                              "ms_min": round(min(t), 3), "ms_max": round(max(t), 3),
                              "vs_d2": round(med[k] / med["(d2) lane order"], 3)}), flush=True)
        print(json.dumps({
            "ids": how, "d2_spread_ms": round(spread["(d2) lane order"], 3),
            "ge_below_d2_by_ms": round(med["(d2) lane order"] - med["(g)+(e)"], 3),
            "claim_1_met": bool(med["(d2) lane order"] - med["(g)+(e)"] > spread["(d2) lane order"]),
            "table_spread_ms": round(spread["(t) table calls by hand"], 3),
            "e_minus_table_ms": round(med["(e) plan order"] - med["(t) table calls by hand"], 3),
            "claim_2_met": bool(abs(med["(e) plan order"] - med["(t) table calls by hand"]) <=
                                spread["(t) table calls by hand"])}), flush=True)

        # the gather alone, in its two shapes
        def shaped(shape):
            def run():
                lib.bbm_hip_set_gather_shape(shape)
                plan.gather(normal, din, dout, xi)
            return run
        times = time_variants({"gather, a stream at a time": shaped(0), "gather, batched": shaped(1)}, a.reps, a.warmup)
        lib.bbm_hip_set_gather_shape(0)
        for k, t in times.items():
            print(json.dumps({"ids": how, "lanes": n, "variant": k, "reps": len(t),
                              "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3),
                              "ms_max": round(max(t), 3)}), flush=True)
        del s_normal, s_in, s_out, s_xi, slices
        plan.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
