"""The world-space eval_pdf call against the staged three-launch pipeline and the local call alone: ms per call and
algorithmic TB/s.

  python tools/bench_frame_eval.py [--lanes 100000000] [--heavy-lanes 10000000] [--reps 25] [--warmup 5]

Per workload four variants, through the C-ABI on resident, 16-byte aligned buffers:
  (a) local: bbm_hip_eval_pdf on local directions -- 40 B / lane; what next-event estimation would cost if the
      renderer's directions were local already (first row: the base of `vs_uniform`);
  (b) staged: bbm_hip_frame_to_local on `in` (36 B), on `out` (36 B), bbm_hip_eval_pdf -- three launches, 112 B;
  (c) fused: bbm_hip_eval_pdf_world -- one launch, 52 B per lane (the normal is 12 B more than (a));
  (d) fused with the cosine -- 56 B.
Workloads: CookTorrance and GGX at --lanes; the CookTorrance material table (4 B / lane more on every variant) with
M = 16 and 1 024 materials and random indices; He, the compaction kernel, at --heavy-lanes.  Normals are random unit
vectors; `in` and `out` are upper-hemisphere local directions taken to world space by bbm_hip_frame_to_global, so
every lane evaluates the model, and (a) runs on those local directions.  Each variant is timed with HIP events on the
launch stream, the variants of a workload interleaved launch by launch after a warm-up; the median and the range over
--reps are reported, then (c) / (b) and (c) / (a) beside the byte ratios.  The byte counts are the arrays a call reads
and writes once.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from bbm_amd import _lib  # noqa: E402
from tools.bench_table import cooktorrance_ramp, indices  # noqa: E402
from tools.bench_varying import report  # noqa: E402

LOCAL, STAGED, FUSED, FUSED_COS = "local eval_pdf", "staged, three launches", "fused world", "fused world + cosine"


class Buffers:
    """Inputs and every output of the four variants for n lanes (n a multiple of 4: every row 16-byte aligned)."""

    def __init__(self, n):
        assert n % 4 == 0
        self.n = n
        self.normal = bbm_amd.fill_directions(0xF4A3E, 2, 0, n, mode=1)           # the whole sphere
        self.local_in = bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=0)        # the upper hemisphere
        self.local_out = bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=0)
        self.din = bbm_amd.to_global(self.normal, self.local_in)
        self.dout = bbm_amd.to_global(self.normal, self.local_out)
        self.staged_in = torch.empty((3, n), dtype=torch.float32, device="cuda")
        self.staged_out = torch.empty((3, n), dtype=torch.float32, device="cuda")
        self.rgb = torch.empty((3, n), dtype=torch.float32, device="cuda")
        self.pdf = torch.empty((n,), dtype=torch.float32, device="cuda")
        self.cos = torch.empty((n,), dtype=torch.float32, device="cuda")

    @staticmethod
    def rows(t):
        return [t[k].data_ptr() for k in range(t.shape[0])]


def variants_of(b, head, table=False):
    """head: the leading arguments of the calls (model id, parameters, count; or table, flags, indices)."""
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    nrm = b.rows(b.normal)
    tail = [None, b.n, 3, 0] + b.rows(b.rgb) + [b.pdf.data_ptr()]
    local = lib.bbm_hip_eval_pdf_table if table else lib.bbm_hip_eval_pdf
    world = lib.bbm_hip_eval_pdf_table_world if table else lib.bbm_hip_eval_pdf_world

    def local_alone():
        _lib.check(local(*head, *b.rows(b.local_in), *b.rows(b.local_out), *tail, s))

    def staged():
        _lib.check(lib.bbm_hip_frame_to_local(*nrm, *b.rows(b.din), None, b.n, *b.rows(b.staged_in), s))
        _lib.check(lib.bbm_hip_frame_to_local(*nrm, *b.rows(b.dout), None, b.n, *b.rows(b.staged_out), s))
        _lib.check(local(*head, *b.rows(b.staged_in), *b.rows(b.staged_out), *tail, s))

    def fused():
        _lib.check(world(*head, *nrm, *b.rows(b.din), *b.rows(b.dout), *tail, None, s))

    def fused_cos():
        _lib.check(world(*head, *nrm, *b.rows(b.din), *b.rows(b.dout), *tail, b.cos.data_ptr(), s))
    return {LOCAL: local_alone, STAGED: staged, FUSED: fused, FUSED_COS: fused_cos}


def run(label, b, head, reps, warmup, table=False):
    extra = 4 if table else 0
    nbytes = {LOCAL: 40 + extra, STAGED: 112 + extra, FUSED: 52 + extra, FUSED_COS: 56 + extra}
    rows = {r["variant"]: r for r in report(label, b.n, variants_of(b, head, table), nbytes, reps, warmup)}
    a, st, fu = rows[LOCAL], rows[STAGED], rows[FUSED]
    print(json.dumps({
        "model": label, "fused_vs_staged": round(fu["ms_median"] / st["ms_median"], 3),
        "bytes_fused_vs_staged": round(nbytes[FUSED] / nbytes[STAGED], 3),
        "fused_vs_local": round(fu["ms_median"] / a["ms_median"], 3),
        "bytes_fused_vs_local": round(nbytes[FUSED] / nbytes[LOCAL], 3),
        "staged_spread_ms": round(st["ms_max"] - st["ms_min"], 4),
        "fused_wins_by_more_than_staged_spread": bool(st["ms_median"] - fu["ms_median"] > st["ms_max"] - st["ms_min"]),
    }), flush=True)


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
    run("CookTorrance", b, head_of(bbm_amd.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5)), a.reps, a.warmup)
    run("GGX", b, head_of(bbm_amd.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.3, eta=1.4)), a.reps, a.warmup)
    for count in (16, 1024):
        table = bbm_amd.MaterialTable("CookTorrance", cooktorrance_ramp(count))
        rnd, srt = indices(count, a.lanes, count)
        del srt
        run(f"CookTorrance table M={count} random", b, [table._live(), 0, rnd.data_ptr()], a.reps, a.warmup, table=True)
        del rnd
        table.close()
    del b

    b = Buffers(a.heavy_lanes)
    run("He", b, head_of(bbm_amd.BsdfModel("He")), a.reps, a.warmup)


if __name__ == "__main__":
    main()
