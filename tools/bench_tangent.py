"""The tangent forms of the world-space calls against the staged three-launch pipeline with the tangent frame calls and
against the normal-only fused call: ms per call and algorithmic TB/s.

  python tools/bench_tangent.py [--lanes 100000000] [--reps 25] [--warmup 5]

Per model (Ward and GGXHeitz, both with unequal x / y roughness) and per call three variants, through the C-ABI on
resident, 16-byte aligned buffers:
  (a) normal-only: the fused world call without a tangent -- what the tangent's 12 B per lane are added to;
  (b) staged: the tangent frame calls around the local call, three launches;
  (c) fused: the *_tangent call, one launch.
Calls and bytes per lane (the arrays a call reads and writes once):
  sample_eval, weight only   (a) 64    (b) to_local_tangent 48 + local 52 + to_global_tangent 48 = 148    (c) 76
  eval_pdf with the cosine   (a) 56    (b) to_local_tangent 48 + 48 + local 40 = 136                      (c) 68
Normals and tangents are random unit vectors (two different streams: a tangent is parallel to its normal on no lane
to speak of); `out` and `in` are upper-hemisphere local directions taken to world space in the tangent frame, so every
lane evaluates the model.  Each variant is timed with HIP events on the launch stream, the variants of a call
interleaved launch by launch after a warm-up; the median and the range over --reps are reported, then whether (c)
beats (b) by more than (b)'s own min-max spread.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bbm_amd  # noqa: E402
from bbm_amd import _lib  # noqa: E402
from tools.bench_varying import report  # noqa: E402

PLAIN, STAGED, FUSED = "normal-only fused", "staged, three launches, tangent frames", "fused tangent"


class Buffers:
    """Inputs and every output of the variants for n lanes (n a multiple of 4: every row 16-byte aligned)."""

    def __init__(self, n):
        assert n % 4 == 0
        self.n = n
        self.normal = bbm_amd.fill_directions(0xF4A3E, 2, 0, n, mode=1)           # the whole sphere
        self.tangent = bbm_amd.fill_directions(0x7A46E47, 3, 0, n, mode=1)
        self.din = bbm_amd.to_global(self.normal, bbm_amd.fill_directions(0xBB5EED, 0, 0, n, mode=0), tangent=self.tangent)
        self.dout = bbm_amd.to_global(self.normal, bbm_amd.fill_directions(0xBB5EED, 1, 0, n, mode=0), tangent=self.tangent)
        self.xi = torch.rand((2, n), dtype=torch.float32, device="cuda")
        f32 = dict(dtype=torch.float32, device="cuda")
        self.staged_a = torch.empty((3, n), **f32)
        self.staged_b = torch.empty((3, n), **f32)
        self.dir = torch.empty((3, n), **f32)
        self.rgb = torch.empty((3, n), **f32)      # eval_pdf's value, sample_eval's weight
        self.pdf = torch.empty((n,), **f32)
        self.cos = torch.empty((n,), **f32)
        self.flag = torch.empty((n,), dtype=torch.int32, device="cuda")

    @staticmethod
    def rows(t):
        return [t[k].data_ptr() for k in range(t.shape[0])]


def sample_eval_variants(b, head):
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    nrm, tan = b.rows(b.normal), b.rows(b.tangent)
    mid = [b.xi[0].data_ptr(), b.xi[1].data_ptr(), None, b.n, 3, 0]
    weight_only = [b.pdf.data_ptr(), b.flag.data_ptr(), None, None, None] + b.rows(b.rgb)

    def plain():
        _lib.check(lib.bbm_hip_sample_eval_world(*head, *nrm, *b.rows(b.dout), *mid, *b.rows(b.dir), *weight_only, s))

    def staged():
        _lib.check(lib.bbm_hip_frame_to_local_tangent(*nrm, *tan, *b.rows(b.dout), None, b.n, *b.rows(b.staged_a), s))
        _lib.check(lib.bbm_hip_sample_eval(*head, *b.rows(b.staged_a), *mid, *b.rows(b.staged_b), *weight_only, s))
        _lib.check(lib.bbm_hip_frame_to_global_tangent(*nrm, *tan, *b.rows(b.staged_b), None, b.n, *b.rows(b.dir), s))

    def fused():
        _lib.check(lib.bbm_hip_sample_eval_world_tangent(*head, *nrm, *tan, *b.rows(b.dout), *mid, *b.rows(b.dir),
                                                         *weight_only, s))
    return {PLAIN: plain, STAGED: staged, FUSED: fused}, {PLAIN: 64, STAGED: 148, FUSED: 76}


def eval_pdf_variants(b, head):
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    nrm, tan = b.rows(b.normal), b.rows(b.tangent)
    tail = [None, b.n, 3, 0] + b.rows(b.rgb) + [b.pdf.data_ptr()]

    def plain():
        _lib.check(lib.bbm_hip_eval_pdf_world(*head, *nrm, *b.rows(b.din), *b.rows(b.dout), *tail, b.cos.data_ptr(), s))

    def staged():       # the cosine is the z row of the first call's output: nothing more to move
        _lib.check(lib.bbm_hip_frame_to_local_tangent(*nrm, *tan, *b.rows(b.din), None, b.n, *b.rows(b.staged_a), s))
        _lib.check(lib.bbm_hip_frame_to_local_tangent(*nrm, *tan, *b.rows(b.dout), None, b.n, *b.rows(b.staged_b), s))
        _lib.check(lib.bbm_hip_eval_pdf(*head, *b.rows(b.staged_a), *b.rows(b.staged_b), *tail, s))

    def fused():
        _lib.check(lib.bbm_hip_eval_pdf_world_tangent(*head, *nrm, *tan, *b.rows(b.din), *b.rows(b.dout), *tail,
                                                      b.cos.data_ptr(), s))
    return {PLAIN: plain, STAGED: staged, FUSED: fused}, {PLAIN: 56, STAGED: 136, FUSED: 68}


def run(label, b, variants, nbytes, reps, warmup):
    rows = {r["variant"]: r for r in report(label, b.n, variants, nbytes, reps, warmup)}
    pl, st, fu = rows[PLAIN], rows[STAGED], rows[FUSED]
    print(json.dumps({
        "case": label, "fused_vs_staged": round(fu["ms_median"] / st["ms_median"], 3),
        "bytes_fused_vs_staged": round(nbytes[FUSED] / nbytes[STAGED], 3),
        "fused_vs_normal_only": round(fu["ms_median"] / pl["ms_median"], 3),
        "bytes_fused_vs_normal_only": round(nbytes[FUSED] / nbytes[PLAIN], 3),
        "staged_spread_ms": round(st["ms_max"] - st["ms_min"], 4),
        "fused_wins_by_more_than_staged_spread": bool(st["ms_median"] - fu["ms_median"] > st["ms_max"] - st["ms_min"]),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.lanes % 4:
        ap.error("--lanes must be a multiple of 4")
    torch.cuda.set_device(0)
    print('{"device": "%s"}' % torch.cuda.get_device_name(0), flush=True)
    b = Buffers(a.lanes)
    models = [bbm_amd.Ward(albedo=[0.3, 0.5, 0.7], roughness=[0.1, 0.4]),
              bbm_amd.GGXHeitz(albedo=[0.7, 0.6, 0.5], roughness=[0.15, 0.45], eta=1.4)]
    for m in models:
        assert m.anisotropic
        head = [m.model_id, m._pptr(), m._params.size]
        run(f"{m.name} sample_eval, weight only", b, *sample_eval_variants(b, head), a.reps, a.warmup)
        run(f"{m.name} eval_pdf with the cosine", b, *eval_pdf_variants(b, head), a.reps, a.warmup)


if __name__ == "__main__":
    main()
