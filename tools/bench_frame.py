"""The world-space sample_eval call against the staged three-launch pipeline and the local call alone: ms per bounce
and algorithmic TB/s.

  python tools/bench_frame.py [--lanes 100000000] [--reps 25] [--warmup 5]

Per workload three variants, through the C-ABI on resident, 16-byte aligned buffers:
  (a) local: bbm_hip_sample_eval on local directions -- 52 B / lane with the weight alone, 64 B with the value too;
      what a bounce would cost if the renderer's directions were local already (first row: the ratios' base);
  (b) staged: bbm_hip_frame_to_local (36 B), bbm_hip_sample_eval, bbm_hip_frame_to_global (36 B) -- three launches,
      124 / 136 B per lane;
  (c) fused: bbm_hip_sample_eval_world -- one launch, 64 / 76 B per lane (the normal is 12 B more than (a)).
Workloads: CookTorrance and GGX, weight alone and value + weight.  Normals are random unit vectors, `out` covers the
upper hemisphere of world space, xi is uniform.  Each variant is timed with HIP events on the launch stream, the
variants of a workload interleaved launch by launch after a warm-up; the median and the range over --reps are
reported.  The byte counts are the arrays a call reads and writes once.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from bbm_amd import _lib  # noqa: E402
from tools.bench_sample_eval import Buffers  # noqa: E402
from tools.bench_varying import report  # noqa: E402


def variants_of(b, normal, local, world_dir, head, value):
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    nrm, out = b.rows(normal), b.rows(b.out)
    xi_tail = b.rows(b.xi) + [None, b.n, 3, 0]
    outs = [b.pdf.data_ptr(), b.flag.data_ptr()] + (b.rows(b.value) if value else [None] * 3) + b.rows(b.weight)

    def local_alone():
        _lib.check(lib.bbm_hip_sample_eval(*head, *out, *xi_tail, *b.rows(b.dir), *outs, s))

    def staged():
        _lib.check(lib.bbm_hip_frame_to_local(*nrm, *out, None, b.n, *b.rows(local), s))
        _lib.check(lib.bbm_hip_sample_eval(*head, *b.rows(local), *xi_tail, *b.rows(b.dir), *outs, s))
        _lib.check(lib.bbm_hip_frame_to_global(*nrm, *b.rows(b.dir), None, b.n, *b.rows(world_dir), s))

    def fused():
        _lib.check(lib.bbm_hip_sample_eval_world(*head, *nrm, *out, *xi_tail, *b.rows(world_dir), *outs, s))
    return {"local sample_eval": local_alone, "staged, three launches": staged, "fused world": fused}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.lanes % 4:
        ap.error("the lane count must be a multiple of 4")
    torch.cuda.set_device(0)
    print('{"device": "%s"}' % torch.cuda.get_device_name(0), flush=True)

    b = Buffers(a.lanes)
    normal = bbm_amd.fill_directions(0xF4A3E, 2, 0, a.lanes, mode=1)          # the whole sphere
    local = torch.empty((3, a.lanes), dtype=torch.float32, device="cuda")
    world_dir = torch.empty((3, a.lanes), dtype=torch.float32, device="cuda")
    models = {"CookTorrance": bbm_amd.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5),
              "GGX": bbm_amd.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.3, eta=1.4)}
    for name, m in models.items():
        head = [m.model_id, m._pptr(), m._params.size]
        for value in (False, True):
            extra = 12 if value else 0
            nbytes = {"local sample_eval": 52 + extra, "staged, three launches": 124 + extra, "fused world": 64 + extra}
            report(f"{name}, {'value + weight' if value else 'weight'}", b.n,
                   variants_of(b, normal, local, world_dir, head, value), nbytes, a.reps, a.warmup)


if __name__ == "__main__":
    main()
