"""Edge-of-the-box parameter sets and lobe-centred direction pairs (tests/test_edge_params_host.py on the CPU,
tests/test_gpu_edge_params.py on the GPU).  A plain helper: no fixtures, reference-side only.

ladder(name)     the row's parameter sets at and next to the faces of its box, from tests/golden/models.json;
lobe_pairs()     224 (in, out) pairs within 0 .. 0.5 of the mirror and the retro direction of eight `out`;
classify(...)    the lanes on which the reference itself leaves the parity bar when its inputs move by one float step.
"""
import re

import numpy as np

from tests import oracle_util as ou

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
HI_UNBOUNDED = 1e6                   # hi* of a parameter whose upper bound is FLT_MAX (or not finite)
STEPS = (2, 4, 6)                    # lo + (hi* - lo) 10^-k
TRIALS = 8                           # classify: moved copies of the inputs
SEED = 20261020

_TOKEN = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[A-Za-z_]\w*|\[|\]")


def box(name):
    """(defaults, lo, hi*) of the row as float64 arrays holding float32 values."""
    m = ou.golden_meta()["models"][name]
    lo = np.asarray(m["lower"], np.float64)
    hi = np.asarray(m["upper"], np.float64)
    hi = np.where(np.isfinite(hi) & (hi < FLT_MAX), hi, HI_UNBOUNDED)
    return np.asarray(m["defaults"], np.float64), lo, hi


def attribute_groups(name):
    """The flat parameter indices of every attribute that has more than one value (an RGB albedo, He's three real
    and three imaginary indices of refraction, Ward's two roughnesses), read off the row's printed default model
    (models.json `strings`[0]): each innermost bracket is one group, in parameter order."""
    m = ou.golden_meta()["models"][name]
    groups, cur, k = [], None, 0
    for tok in _TOKEN.findall(m["strings"][0]):
        if tok == "[":
            cur = []
        elif tok == "]":
            if cur:
                groups.append(cur)
            cur = None
        elif (tok[0].isalpha() or tok[0] == "_") and tok not in ("inf", "nan"):
            continue
        else:
            if cur is not None:
                cur.append(k)
            k += 1
    assert k == m["nparams"], (name, k, m["nparams"])
    return [g for g in groups if len(g) > 1]


def _values(lo, hi):
    """The distinct float32 values of {lo, hi*, lo + (hi* - lo) 10^-k}, tagged."""
    out, seen = [], set()
    for tag, v in [("lo", lo), ("hi", hi)] + [(f"1e-{k}", lo + (hi - lo) * 10.0 ** -k) for k in STEPS]:
        v = F(v)
        if v.tobytes() not in seen:
            seen.add(v.tobytes())
            out.append((tag, v))
    return out


def ladder(name):
    """[(tag, params float32)]: one parameter at a time at each of its edge values (the others at their defaults),
    every multi-valued attribute moved as a whole through the same steps, and the two corners (all lo, all hi*).
    A set that repeats an earlier one is left out.  Tags: "p<j>=lo|hi|1e-k", "a<j0>-<j1>=...", "corner=lo|hi"."""
    d, lo, hi = box(name)
    sets, seen = [], set()

    def add(tag, p):
        p = np.asarray(p, F)
        if p.tobytes() not in seen:
            seen.add(p.tobytes())
            sets.append((tag, p))
    for j in range(d.size):
        for tag, v in _values(lo[j], hi[j]):
            p = d.astype(F)
            p[j] = v
            add(f"p{j}={tag}", p)
    for g in attribute_groups(name):
        for tag in ["lo", "hi"] + [f"1e-{k}" for k in STEPS]:
            p = d.astype(F)
            for j in g:
                v = {"lo": lo[j], "hi": hi[j]}.get(tag)
                p[j] = F(v if v is not None else lo[j] + (hi[j] - lo[j]) * 10.0 ** -int(tag[3:]))
            add(f"a{g[0]}-{g[-1]}={tag}", p)
    add("corner=lo", lo.astype(F))
    add("corner=hi", hi.astype(F))
    return sets


def face_sets(name):
    """The ladder's sets that sample and reflectance run: the two corners and each parameter's lo and hi* set."""
    keep = re.compile(r"^(corner=(lo|hi)|p\d+=(lo|hi))$")
    return [(t, p) for t, p in ladder(name) if keep.match(t)]


def corner_sets(name):
    _, lo, hi = box(name)
    return [("corner=lo", lo.astype(F)), ("corner=hi", hi.astype(F))]


OUT_Z = (1.0, 0.7, 0.1, 1e-3)
OUT_PHI = (0.0, 2.1)
DELTA = (0.0, 1e-7, 1e-5, 1e-3, 1e-2, 1e-1, 0.5)


def lobe_pairs():
    """(din, dout), float32 (3, 224), in this fixed order (slowest first): out z, out azimuth, base (mirror, retro),
    delta, tangent.  in = normalize(base + delta t) with |z| taken; float64 throughout, rounded once."""
    din, dout = [], []
    for z in OUT_Z:
        s = np.sqrt(max(1.0 - z * z, 0.0))
        for phi in OUT_PHI:
            out = np.array([s * np.cos(phi), s * np.sin(phi), z])
            tangents = (np.array([np.cos(phi), np.sin(phi), 0.0]),
                        np.array([np.cos(phi + 1.3), np.sin(phi + 1.3), 0.3]))
            for base in (np.array([-out[0], -out[1], out[2]]), out):
                for delta in DELTA:
                    for t in tangents:
                        v = base + delta * t
                        v = v / np.sqrt((v * v).sum())
                        v[2] = abs(v[2])
                        din.append(v)
                        dout.append(out)
    return np.asarray(din).T.astype(F).copy(), np.asarray(dout).T.astype(F).copy()


def classify(ref_fn, inputs, ref, ok=ou.parity_ok):
    """Boolean (n,) mask of ill-conditioned lanes, from the reference alone: a lane on which any of TRIALS seeded
    moves of every input coordinate by -1, 0 or +1 float steps takes the reference's own output (ref_fn(*inputs) ->
    (c, n)) outside `ok` of `ref`.  ok: oracle_util.parity_ok, or parity_ok_f64 for a double reference."""
    inputs = [np.asarray(a, F) for a in inputs]
    ref = np.asarray(ref)
    n = ref.shape[-1]
    rng = np.random.default_rng(SEED)
    moved = []
    for a in inputs:
        st = rng.integers(-1, 2, size=(TRIALS,) + a.shape)
        moved.append(np.ascontiguousarray(np.concatenate([ou.perturb_ulps(a, st[t]) for t in range(TRIALS)], axis=1)))
    r = np.asarray(ref_fn(*moved)).reshape(ref.shape[0], TRIALS, n)
    return ~ok(r, ref[:, None, :]).all(axis=(0, 1))


def normal_lanes(ref, tiny=ou.FLT_MIN):
    """Lanes whose reference value is finite in every channel and normal (|ref| >= tiny) in at least one: the lanes
    on which a comparison is more than zero against zero."""
    ref = np.asarray(ref, np.float64)
    return np.isfinite(ref).all(0) & (np.abs(ref) >= tiny).any(0)
