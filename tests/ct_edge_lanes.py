"""Direction pairs aimed at the edges of CookTorrance's per-pair arithmetic (tests/test_gpu_ct_edges.py).  A plain
helper: no fixtures, reference-side only.

The 1 M-pair parity batches draw random directions, which almost never reach the operands at which a special-case
select of a quotient or a root decides the result.  lanes() builds N = 4 x 256 x 2 + 3 pairs (two full workgroups
of the four-pair kernel and its one-pair tail) out of:
  * z(in) and z(out) over {0, +-FLT_MIN, 1e-20, 1}, all 25 combinations;
  * in == out and in == mirror(out) at z from 1 down to FLT_MIN;
  * grazing pairs a quarter turn apart, whose halfway vector has z(h) = sqrt(2) z from 1e-3 down to 1e-19 -- cos^2 is
    then subnormal and the Beckmann exponent far below expf's underflow;
  * pairs 0 .. 1e-3 rad off the mirror direction at normal incidence (Fresnel's c -> 1, tan(theta) -> 0);
  * lower-hemisphere pairs and random upper-hemisphere pairs.
All directions are finite unit vectors (to float rounding).  mask() switches every 7th lane off.

The reference alone decides which lanes stay: a lane on which it returns a non-finite value for any of the
parameter sets is replaced by a plain pair (lanes() returns how many; the test bounds them at 1 %).
"""
import numpy as np

from tests import oracle_util as ou

F = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
N = 4 * 256 * 2 + 3
NAME = "CookTorrance"
SEED = 20261021


def param_sets():
    """[(tag, params)]: roughness and eta at both ends of their boxes and at the benchmark's values (the model's
    defaults), albedo at its default."""
    m = ou.golden_meta()["models"][NAME]
    d, lo, hi = (np.asarray(m[k], np.float64) for k in ("defaults", "lower", "upper"))
    sets = []
    for rt, r in (("lo", lo[3]), ("bench", d[3]), ("hi", hi[3])):
        for et, e in (("lo", lo[4]), ("bench", d[4]), ("hi", hi[4])):
            sets.append((f"roughness={rt},eta={et}", np.asarray([d[0], d[1], d[2], r, e], F)))
    return sets


def _dir(z, phi):
    z = np.asarray(z, np.float64)
    s = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z + 0 * phi])


def _mirror(d):
    return np.stack([-d[0], -d[1], d[2]])


def _raw():
    rng = np.random.default_rng(SEED)
    ins, outs = [], []

    def add(i, o):
        ins.append(np.asarray(i, np.float64).reshape(3, -1))
        outs.append(np.asarray(o, np.float64).reshape(3, -1))
    zs = [0.0, FLT_MIN, -FLT_MIN, 1e-20, 1.0]
    for zi in zs:
        for zo in zs:
            add(_dir(zi, rng.uniform(0, 2 * np.pi)), _dir(zo, rng.uniform(0, 2 * np.pi)))
    zl = np.asarray([1.0, 0.999, 0.7, 0.1, 1e-3, 1e-8, 1e-19, 1e-20, 1e-30, FLT_MIN])
    phi = rng.uniform(0, 2 * np.pi, zl.size)
    add(_dir(zl, phi), _dir(zl, phi))                       # in == out
    add(_mirror(_dir(zl, phi)), _dir(zl, phi))              # in == mirror(out)
    eps = np.asarray([1e-3, 1e-5, 1e-8, 1e-10, 1e-15, 1e-17, 1e-18, 3e-19, 1e-19]) / np.sqrt(2.0)
    for e in eps:                                           # z(h) = sqrt(2) e
        p = rng.uniform(0, 2 * np.pi)
        add(_dir(e, p), _dir(e, p + np.pi / 2))
        add(_dir(e, p), _dir(1e-3, p + np.pi / 2))
    for t in (0.0, 1e-7, 1e-5, 1e-3):                       # near the mirror direction, near normal incidence
        for t0 in (0.0, 1e-4, 0.3):
            p = rng.uniform(0, 2 * np.pi)
            o = _dir(np.cos(t0), p)
            add(_mirror(_dir(np.cos(t0 + t), p)), o)
    k = 200                                                 # lower hemisphere: in, out, both
    for si, so in ((-1, 1), (1, -1), (-1, -1)):
        add(_dir(si * rng.uniform(0, 1, k), rng.uniform(0, 2 * np.pi, k)),
            _dir(so * rng.uniform(0, 1, k), rng.uniform(0, 2 * np.pi, k)))
    have = sum(a.shape[1] for a in ins)
    k = N - have
    assert k > 256, k
    add(_dir(rng.uniform(0, 1, k), rng.uniform(0, 2 * np.pi, k)), _dir(rng.uniform(0, 1, k), rng.uniform(0, 2 * np.pi, k)))
    din, dout = np.concatenate(ins, 1).astype(F), np.concatenate(outs, 1).astype(F)
    perm = rng.permutation(N)                               # every kind of lane in both workgroups and the tail
    return np.ascontiguousarray(din[:, perm]), np.ascontiguousarray(dout[:, perm])


_CACHE = {}


def lanes():
    """(din, dout, refs, dropped): (3, N) float32 directions, {tag: (4, N) reference eval RGB + pdf} for
    param_sets(), and the number of lanes replaced because the reference was not finite there."""
    if "v" not in _CACHE:
        din, dout = _raw()
        sets = param_sets()
        bad = np.zeros(N, bool)
        for _, p in sets:
            bad |= ~np.isfinite(ou.oracle_eval_pdf(NAME, p, din, dout)).all(0)
        din[:, bad] = np.asarray([[0.6], [0.0], [0.8]], F)
        dout[:, bad] = np.asarray([[0.0], [0.6], [0.8]], F)
        refs = {t: ou.oracle_eval_pdf(NAME, p, din, dout) for t, p in sets}
        for r in refs.values():
            assert np.isfinite(r).all()
            r.setflags(write=False)
        din.setflags(write=False)
        dout.setflags(write=False)
        _CACHE["v"] = (din, dout, refs, int(bad.sum()))
    return _CACHE["v"]


def mask():
    m = np.ones(N, np.uint8)
    m[::7] = 0
    return m
