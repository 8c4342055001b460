"""The fused sample_eval call against the staged pair of launches: ms per call and algorithmic TB/s (DESIGN.md
section 4.16).

  python tools/bench_sample_eval.py [--lanes 100000000] [--heavy-lanes 10000000] [--reps 25] [--warmup 5]

Per workload three variants, through the C-ABI on resident, 16-byte aligned buffers:
  (a) staged: bbm_hip_sample, then bbm_hip_eval at the sampled direction -- two launches, 76 B / lane (sample 20 in +
      20 out, eval 24 in + 12 out); the yardstick, kernels this call does not touch;
  (b) fused, weight alone: bbm_hip_sample_eval with the value group NULL -- 52 B / lane;
  (c) fused, value and weight -- 64 B / lane.
Workloads: CookTorrance and GGX at --lanes; Aggregate<Lambertian,Bagher> and He at --heavy-lanes; the CookTorrance
material table (4 B / lane more on every variant: 80 / 56 / 68) with M = 16 and 1 024 materials, random and sorted
indices.  `out` covers the upper hemisphere, xi is uniform.  Each variant is timed with HIP events on the launch stream,
the variants of a workload interleaved launch by launch after a warm-up; the median and the range over --reps are
reported.  The byte counts are the arrays a call reads and writes once.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from bbm_amd import _lib  # noqa: E402
from tools.bench_table import cooktorrance_ramp, indices  # noqa: E402
from tools.bench_varying import report  # noqa: E402


class Buffers:
    """Inputs and every output of the three variants for n lanes (n a multiple of 4: every row 16-byte aligned)."""

    def __init__(self, n):
        assert n % 4 == 0
        self.n = n
        self.out = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=0)
        g = torch.Generator(device="cuda")
        g.manual_seed(0xBB5EED)
        self.xi = torch.rand((2, n), dtype=torch.float32, device="cuda", generator=g)
        self.dir = torch.empty((3, n), dtype=torch.float32, device="cuda")
        self.pdf = torch.empty((n,), dtype=torch.float32, device="cuda")
        self.flag = torch.empty((n,), dtype=torch.int32, device="cuda")
        self.value = torch.empty((3, n), dtype=torch.float32, device="cuda")
        self.weight = torch.empty((3, n), dtype=torch.float32, device="cuda")

    def rows(self, t):
        return [t[k].data_ptr() for k in range(t.shape[0])]

    def sample_args(self):
        return self.rows(self.out) + self.rows(self.xi) + [None, self.n, 3, 0] + self.rows(self.dir) + \
            [self.pdf.data_ptr(), self.flag.data_ptr()]

    def eval_args(self):
        return self.rows(self.dir) + self.rows(self.out) + [None, self.n, 3, 0] + self.rows(self.value)


def variants_of(b, head, table=False):
    """head: the leading arguments of the calls (model id, parameters, count; or table, flags, indices)."""
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    none3 = [None, None, None]
    if table:
        sample, evalf, fused = lib.bbm_hip_sample_table, lib.bbm_hip_eval_pdf_table, lib.bbm_hip_sample_eval_table
        eval_tail = [None]                                   # eval alone: the pdf pointer is NULL
    else:
        sample, evalf, fused = lib.bbm_hip_sample, lib.bbm_hip_eval, lib.bbm_hip_sample_eval
        eval_tail = []

    def staged():
        _lib.check(sample(*head, *b.sample_args(), s))
        _lib.check(evalf(*head, *b.eval_args(), *eval_tail, s))

    def fused_weight():
        _lib.check(fused(*head, *b.sample_args(), *none3, *b.rows(b.weight), s))

    def fused_both():
        _lib.check(fused(*head, *b.sample_args(), *b.rows(b.value), *b.rows(b.weight), s))
    return {"staged sample + eval": staged, "fused, weight": fused_weight, "fused, value + weight": fused_both}


def run(label, b, head, reps, warmup, table=False):
    extra = 4 if table else 0
    nbytes = {"staged sample + eval": 76 + extra, "fused, weight": 52 + extra, "fused, value + weight": 64 + extra}
    return report(label, b.n, variants_of(b, head, table), nbytes, reps, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=100_000_000)
    ap.add_argument("--heavy-lanes", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.lanes % 4 or a.heavy_lanes % 4:
        ap.error("lane counts must be multiples of 4")
    torch.cuda.set_device(0)
    print('{"device": "%s"}' % torch.cuda.get_device_name(0), flush=True)

    def head_of(m):
        return [m.model_id, m._pptr(), m._params.size]

    b = Buffers(a.lanes)
    ct = bbm_amd.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5)
    run("CookTorrance", b, head_of(ct), a.reps, a.warmup)
    ggx = bbm_amd.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.3, eta=1.4)
    run("GGX", b, head_of(ggx), a.reps, a.warmup)
    for count in (16, 1024):
        table = bbm_amd.MaterialTable("CookTorrance", cooktorrance_ramp(count))
        rnd, srt = indices(count, a.lanes, count)
        for label, idx in (("random", rnd), ("sorted", srt)):
            run(f"CookTorrance table M={count} {label}", b, [table._live(), 0, idx.data_ptr()], a.reps, a.warmup,
                table=True)
        del rnd, srt
        table.close()
    del b

    b = Buffers(a.heavy_lanes)
    for name in ("Aggregate<Lambertian,Bagher>", "He"):
        m = bbm_amd.BsdfModel(name)
        run(name, b, head_of(m), a.reps, a.warmup)


if __name__ == "__main__":
    main()
