"""A tangent per lane for the anisotropic models, on the GPU (frame.hpp's tangent_frame; the tangent forms of the
world-space kernels of sample_eval.hpp, eval_world.hpp and lanes.hpp): bbm_hip_frame_to_local_tangent /
_to_global_tangent, bbm_hip_sample_eval(_table)_world_tangent, bbm_hip_eval_pdf(_table)_world_tangent,
bbm_hip_set_eval_pdf_tangent / _set_sample_eval_tangent and the Python `tangent=` surface.

What is held, and to what:
  1. fallback: on every lane whose tangent is not live (computed here in the kernel's float32 order) the tangent frame
     calls equal the normal-only frame calls, bit for bit;
  2. the tangent frame against a float64 numpy restatement of the rule, to_global(to_local(v)) against v, and the
     frame's orthonormality, each within CAP relative to |v| (test_frame_against_float64 says where CAP comes from);
  3. the exact permutation frame: normal (0, 0, 1) and tangent (0, 1, 0) make the world call the local call at
     (v.y, -v.x, v.z) (`==`: -0 equals 0), and turn Ward's lobe against the normal-only call;
  4. fused equals staged -- the tangent frame calls around the local call -- bit for bit on every output array, for the
     nine anisotropic rows, uniform and table call;
  5. the other 40 rows (34 with tables) ignore the tangent: the tangent call is the normal-only call, bit for bit;
  6. a set's lane is the matching table call's lane;
  7. the Python surface returns the C-ABI results.
"Bit for bit" = equal int32 views; NaN lanes compare by where they are NaN.  Every C-ABI call takes its arrays out of
test_gpu_frame's sentinel-filled arena, 16-byte aligned (the quad kernels and their scalar tail) or 4 bytes further (the
one-lane kernels); whatever lies outside the call's output arrays must be unchanged afterwards.

The normals are test_gpu_frame's.  The tangents (TANGENT): random vectors of mixed length, with these lanes replaced,
one per kind, among the first eight lanes and once more on lane 256 (the scalar tail of n = 257): t = 0, t = n,
t = -3 n, a NaN component, |t| = 1e-5, |t| = 1e3, t exactly perpendicular to n.
"""
import numpy as np
import pytest

import bbm_amd
from tests import test_gpu_frame as tf
from tests import test_gpu_frame_eval as te
from tests.test_gpu_frame import Arena, same_bits, same_results, live_lanes, stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(np.finfo(np.float32).eps)
N = 1217
SEED = 0x7A46E47
SHAPES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1217]
NAMES = bbm_amd.model_names()
ANISOTROPIC = ["Ward", "WardDuer", "WardDuerGeislerMoroder", "CookTorranceHeitz", "GGXHeitz", "RibardiereAnisotropic",
               "Lafortune", "AshikhminShirley", "AshikhminShirleyFull"]
ISOTROPIC = [n for n in NAMES if n not in ANISOTROPIC]
ISOTROPIC_TABLES = [n for n in ISOTROPIC if n in tf.SUPPORTED]
SOUTS = tf.OUTS
EOUTS = te.OUTS
CAP = 2.0 ** -18


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


merl = tf.merl


# ------------------------------------------------------------------------ shared inputs (computed once, never written)

def perpendicular(n):
    """A float32 vector whose float32 dot3 with n is exactly 0: two components of n swapped, one negated."""
    return np.array([n[1], -n[0], 0], F) if (n[0] != 0 or n[1] != 0) else np.array([1, 0, 0], F)


def make_tangents(rng, normal):
    n = normal.shape[1]
    t = (rng.standard_normal((3, n)) * np.exp(rng.uniform(-3, 3, n))).astype(F)
    unit = rng.standard_normal((3, n))
    unit = (unit / np.linalg.norm(unit, axis=0)).astype(F)
    # lanes 0 and 1 are the normals (0, 0, 1) and (0, 0, -1), lane 2 has no normal, lanes 3 .. 7 are ordinary ones
    t[:, 0] = 0
    t[:, 1] = normal[:, 1]
    t[:, 3] = F(-3) * normal[:, 3]
    t[1, 4] = np.nan
    t[:, 5] = unit[:, 5] * F(1e-5)
    t[:, 6] = unit[:, 6] * F(1e3)
    t[:, 7] = perpendicular(normal[:, 7])
    t[:, 256] = 0                                  # its normal is (0, 0, 0) too; 257 .. 263: once more on live normals
    t[:, 257] = 0
    t[:, 258] = normal[:, 258]
    t[:, 259] = F(-3) * normal[:, 259]
    t[2, 260] = np.nan
    t[:, 261] = unit[:, 261] * F(1e-5)
    t[:, 262] = unit[:, 262] * F(1e3)
    t[:, 263] = perpendicular(normal[:, 263])
    for a in t:
        a.flags.writeable = False
    return t


def dot32(a, b):
    """dot3 of math.hpp: ((0 + ax bx) + ay by) + az bz, every operation rounded to float32."""
    with np.errstate(all="ignore"):
        return ((F(0) + a[0] * b[0]).astype(F) + (a[1] * b[1]).astype(F)).astype(F) + (a[2] * b[2]).astype(F)


def frame_np(normal, tangent, dt):
    """tangent_frame of frame.hpp in numpy at precision dt, in its operation order, on lanes where the normal and the
    tangent are live -> X, Y, Z (3, n) each."""
    n, t = normal.astype(dt), tangent.astype(dt)
    one = dt(1)

    def dot(a, b):
        return ((dt(0) + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]
    with np.errstate(all="ignore"):
        Z = n * (one / np.sqrt(dot(n, n)))
        d = dot(Z, t)
        p = t - Z * d
        X = p * (one / np.sqrt(dot(p, p)))
        Y = np.stack([Z[1] * X[2] - Z[2] * X[1], Z[2] * X[0] - Z[0] * X[2], Z[0] * X[1] - Z[1] * X[0]])
    return X.astype(dt), Y.astype(dt), Z.astype(dt)


def to_local_np(fr, v, dt):
    X, Y, Z = fr
    v = v.astype(dt)
    dot = lambda a, b: ((dt(0) + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2]
    return np.stack([dot(X, v), dot(Y, v), dot(Z, v)])


def to_global_np(fr, v, dt):
    X, Y, Z = fr
    v = v.astype(dt)
    return np.stack([(X[k] * v[0] + Y[k] * v[1]) + Z[k] * v[2] for k in range(3)])


def tangent_live(normal, tangent):
    """pp > epsilon in the kernel's float32 order (a NaN is not live); the normal's own liveness is live_lanes."""
    with np.errstate(all="ignore"):
        nn = dot32(normal, normal)
        Z = (normal * (F(1) / np.sqrt(nn)).astype(F)).astype(F)
        d = dot32(Z, tangent)
        p = (tangent - (Z * d).astype(F)).astype(F)
        return dot32(p, p) > EPS


_RNG = np.random.default_rng(SEED)
NORMAL = tf.make_normals(np.random.default_rng(tf.SEED), N)
TANGENT = make_tangents(_RNG, NORMAL)
DIN, DOUT = te.make_direction(_RNG, NORMAL), te.make_direction(_RNG, NORMAL)
XI = _RNG.random((2, N), dtype=F)
VEC = (_RNG.standard_normal((3, N)) * np.exp(_RNG.uniform(-3, 3, N))).astype(F)
MASK = np.ones(N, np.uint8)
MASK[[9, 10, 254, 261, N - 1]] = 0
MATERIAL = _RNG.integers(0, 3, N).astype(np.int64)
MATERIAL[[11, 264]] = -1                                   # out of range: the component is switched off
MATERIAL[[12, 265]] = 3
MATERIAL = MATERIAL.astype(np.uint32)
NLIVE, TLIVE = live_lanes(NORMAL), tangent_live(NORMAL, TANGENT)
for _a in (DIN, DOUT, XI, VEC, MASK, MATERIAL):
    _a.flags.writeable = False


def test_the_tangent_set():
    dead = np.nonzero(NLIVE & ~TLIVE)[0]
    assert set(dead) == {0, 1, 3, 4, 5, 257, 258, 259, 260, 261}, dead
    assert not NLIVE[2] and not NLIVE[256]
    assert TLIVE[6] and TLIVE[7] and TLIVE[262] and TLIVE[263]
    assert dot32(NORMAL[:, [7, 263]], TANGENT[:, [7, 263]]).tolist() == [0, 0]
    lib = bbm_amd._lib.load()
    assert sorted(ANISOTROPIC) == sorted(n for i, n in enumerate(NAMES) if lib.bbm_hip_model_anisotropic(i) == 1)
    assert len(ISOTROPIC) == 40 and len(ISOTROPIC_TABLES) == 34


# ------------------------------------------------------------------------ the calls

def tptrs(a, tangent):
    return [a.ptr(k) for k in ("tx", "ty", "tz")] if tangent is not None else [None, None, None]


def tins(tangent, n):
    return {} if tangent is None else {"tx": tangent[0][:n], "ty": tangent[1][:n], "tz": tangent[2][:n]}


def frame_call(to_local, normal, tangent, v, n, mask=None, shift=0):
    """bbm_hip_frame_to_local_tangent / _to_global_tangent (tangent None: three NULL pointers) -> (3, n)."""
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], **tins(tangent, n),
           "x": v[0][:n], "y": v[1][:n], "z": v[2][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    a = Arena(n, shift, ins, ["rx", "ry", "rz"])
    fn = lib.bbm_hip_frame_to_local_tangent if to_local else lib.bbm_hip_frame_to_global_tangent
    bbm_amd._lib.check(fn(*(a.ptr(k) for k in ("nx", "ny", "nz")), *tptrs(a, tangent), *(a.ptr(k) for k in ("x", "y", "z")),
                          a.ptr("mask") if mask is not None else None, n, a.ptr("rx"), a.ptr("ry"), a.ptr("rz"), stream()))
    r = a.results()
    return np.stack([r["rx"], r["ry"], r["rz"]])


def seval_call(m, normal, tangent, out, xi, n, comp=3, mask=None, value=True, weight=True, shift=0, exact=None,
               material=None):
    """bbm_hip_sample_eval(_table)_world_tangent on the first n lanes (tangent None: three NULL pointers)."""
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], **tins(tangent, n),
           "ox": out[0][:n], "oy": out[1][:n], "oz": out[2][:n], "xi0": xi[0][:n], "xi1": xi[1][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    if material is not None:
        ins["material"] = material[:n]
    given = {k: True for k in SOUTS}
    for k in ("r", "g", "b"):
        given[k] = value
    for k in ("wr", "wg", "wb"):
        given[k] = weight
    a = Arena(n, shift, ins, SOUTS)
    args = [a.ptr(k) for k in ("nx", "ny", "nz")] + tptrs(a, tangent) + [a.ptr(k) for k in ("ox", "oy", "oz", "xi0", "xi1")] + \
        [a.ptr("mask") if mask is not None else None, n, comp, 0] + [a.ptr(k) if given[k] else None for k in SOUTS] + [stream()]
    if material is None:
        rc = lib.bbm_hip_sample_eval_world_tangent(m._call_id(exact), m._pptr(), m._params.size, *args)
    else:
        rc = lib.bbm_hip_sample_eval_table_world_tangent(m._live(), m._flags(exact), a.ptr("material"), *args)
    bbm_amd._lib.check(rc)
    return a.results(given)


def eval_call(m, normal, tangent, din, dout, n, comp=3, mask=None, mode=3, cos=True, shift=0, exact=None, material=None):
    """bbm_hip_eval_pdf(_table)_world_tangent on the first n lanes (tangent None: three NULL pointers)."""
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], **tins(tangent, n),
           "ix": din[0][:n], "iy": din[1][:n], "iz": din[2][:n], "ox": dout[0][:n], "oy": dout[1][:n], "oz": dout[2][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    if material is not None:
        ins["material"] = material[:n]
    given = {"r": bool(mode & 1), "g": bool(mode & 1), "b": bool(mode & 1), "pdf": bool(mode & 2), "cos": cos}
    a = Arena(n, shift, ins, EOUTS)
    args = [a.ptr(k) for k in ("nx", "ny", "nz")] + tptrs(a, tangent) + [a.ptr(k) for k in ("ix", "iy", "iz", "ox", "oy", "oz")] + \
        [a.ptr("mask") if mask is not None else None, n, comp, 0] + [a.ptr(k) if given[k] else None for k in EOUTS] + [stream()]
    if material is None:
        rc = lib.bbm_hip_eval_pdf_world_tangent(m._call_id(exact), m._pptr(), m._params.size, *args)
    else:
        rc = lib.bbm_hip_eval_pdf_table_world_tangent(m._live(), m._flags(exact), a.ptr("material"), *args)
    bbm_amd._lib.check(rc)
    return a.results(given)


def staged_mask(n, mask):
    """The staged pipeline's mask: the caller's with the lanes of a normal that is not live cleared.  A tangent that is
    not live masks nothing: its lane runs in the normal-only frame."""
    mk = np.ones(n, np.uint8) if mask is None else mask[:n].copy()
    mk[~NLIVE[:n]] = 0
    return mk


def staged_seval(m, n, mask=None, shift=0, **kw):
    mk = staged_mask(n, mask)
    lo = frame_call(True, NORMAL, TANGENT, DOUT, n, mk, shift)
    res = tf.seval_call(m, None, lo, XI, n, mask=mk, shift=shift, **kw)
    d = frame_call(False, NORMAL, TANGENT, np.stack([res["dx"], res["dy"], res["dz"]]), n, mk, shift)
    res["dx"], res["dy"], res["dz"] = d[0], d[1], d[2]
    return res


def staged_eval(m, n, mask=None, shift=0, cos=True, **kw):
    mk = staged_mask(n, mask)
    li = frame_call(True, NORMAL, TANGENT, DIN, n, mk, shift)
    lo = frame_call(True, NORMAL, TANGENT, DOUT, n, mk, shift)
    res = te.eval_call(m, None, li, lo, n, mask=mk, shift=shift, **kw)
    if cos:
        res["cos"] = li[2]
    return res


# ------------------------------------------------------------------------ 1. fallback

@pytest.mark.parametrize("shift", [0, 1])
def test_fallback_is_the_normal_only_frame(bbm, shift):
    dead = ~TLIVE
    assert dead.sum() >= 12
    for n in SHAPES:
        for to_local in (True, False):
            for mask in (None, MASK):
                got = frame_call(to_local, NORMAL, TANGENT, VEC, n, mask, shift)
                want = tf.frame_call(to_local, NORMAL, VEC, n, mask, shift)
                same_bits(got[:, dead[:n]], want[:, dead[:n]], ("fallback", n, to_local, mask is not None))
                assert np.isfinite(got[:, dead[:n]]).all()
                # three NULL tangent pointers: the call is its counterpart
                same_bits(frame_call(to_local, NORMAL, None, VEC, n, mask, shift), want, ("null tangent", n, to_local))
    # and the frame turns where the tangent is live: the two calls differ on most such lanes
    got, want = frame_call(True, NORMAL, TANGENT, VEC, N, None, shift), tf.frame_call(True, NORMAL, VEC, N, None, shift)
    live = NLIVE & TLIVE
    assert ((got[0] != want[0]) & live).sum() > 0.9 * live.sum()
    same_bits(got[2], want[2], "z does not depend on the tangent")


# ------------------------------------------------------------------------ 2. against float64

def frame_errors(fr, lo, back, v, X, Y, Z):
    """Every quantity test 2 bounds, relative to |v| (the frame's own rows: |v| = 1), against the float64 frame fr."""
    ln = np.linalg.norm(v.astype(np.float64), axis=0)
    dot = lambda a, b: (a.astype(np.float64) * b.astype(np.float64)).sum(0)
    return {
        "to_local": np.abs(lo - to_local_np(fr, v, np.float64)).max(0) / ln,
        "round trip": np.abs(back.astype(np.float64) - v).max(0) / ln,
        "X.Z": np.abs(dot(X, Z)), "Y.Z": np.abs(dot(Y, Z)), "X.Y": np.abs(dot(X, Y)),
        "|X|": np.abs(np.sqrt(dot(X, X)) - 1), "|Y|": np.abs(np.sqrt(dot(Y, Y)) - 1),
    }


def checked_lanes():
    """Normal and tangent live, the tangent at least 30 degrees off the normal (by float64)."""
    n64, t64 = NORMAL.astype(np.float64), TANGENT.astype(np.float64)
    with np.errstate(all="ignore"):
        c = np.abs((n64 * t64).sum(0)) / (np.linalg.norm(n64, axis=0) * np.linalg.norm(t64, axis=0))
    return NLIVE & TLIVE & (c <= np.cos(np.radians(30.0)))


def restatement_errors():
    """The float32 numpy restatement of the rule against float64 over this file's own inputs: the error the format and
    the operation order put between input and output, with nothing of the kernel in it."""
    use = checked_lanes()
    nrm, tan, v = NORMAL[:, use], TANGENT[:, use], VEC[:, use]
    f32, f64 = frame_np(nrm, tan, F), frame_np(nrm, tan, np.float64)
    lo = to_local_np(f32, v, F)
    back = to_global_np(f32, lo, F)
    return frame_errors(f64, lo, back, v, *f32)


def test_cap_is_derived_from_the_restatement():
    worst = max(float(e.max()) for e in restatement_errors().values())
    assert 0 < worst and 4 * worst <= CAP < 8 * worst, (worst, CAP)


@pytest.mark.parametrize("shift", [0, 1])
def test_frame_against_float64(bbm, shift):
    """CAP: the float32 numpy restatement of the rule (frame_np, to_local_np, to_global_np: the kernel's operation
    order) against the float64 one over this file's own lanes differs by at most 5.21e-7 |v| in any of the checked
    quantities (measured on the CPU: to_local 4.27e-7, the round trip 5.21e-7 = 4.4 float32 epsilons, X.Z 4.32e-7,
    Y.Z 6.8e-8, X.Y 7.0e-8, |X| - 1 1.31e-7, |Y| - 1 2.36e-7); 4 x the worst is 2.08e-6, rounded up to a power of two
    CAP = 2^-18 = 3.81e-6
    (test_cap_is_derived_from_the_restatement holds the two together).  A transposed matrix, a wrong handedness or a
    swapped cross product is an O(|v|) error."""
    use = checked_lanes()
    assert use.sum() > 0.8 * N
    unit = [np.tile(np.array(e, F)[:, None], (1, N)) for e in ((1, 0, 0), (0, 1, 0), (0, 0, 1))]
    for n in SHAPES:
        u = use[:n]
        if not u.any():
            continue
        lo = frame_call(True, NORMAL, TANGENT, VEC, n, None, shift)
        back = frame_call(False, NORMAL, TANGENT, lo, n, None, shift)
        X, Y, Z = (frame_call(False, NORMAL, TANGENT, e, n, None, shift)[:, u] for e in unit)   # M e_k: the columns
        fr = frame_np(NORMAL[:, :n][:, u], TANGENT[:, :n][:, u], np.float64)
        errs = frame_errors(fr, lo[:, u], back[:, u], VEC[:, :n][:, u], X, Y, Z)
        for what, e in errs.items():
            print(f"frame vs float64, n={n} shift={shift} {what}: {e.max():.3e} (cap {CAP:.3e})")
            assert e.max() <= CAP, (what, n, e.max())
        # right-handed: X x Y = Z
        cross = np.cross(X.astype(np.float64), Y.astype(np.float64), axis=0)
        assert np.abs(cross - Z).max() <= 4 * CAP, n
        # X lies on the tangent's side
        assert ((X.astype(np.float64) * TANGENT[:, :n][:, u]).sum(0) > 0).all()


# ------------------------------------------------------------------------ 3. the exact permutation frame

@pytest.mark.parametrize("shift", [0, 1])
def test_exact_permutation_frame(bbm, shift):
    """normal (0, 0, 1), tangent (0, 1, 0): X = (0, 1, 0), Y = Z x X = (-1, 0, 0), every product exact; local v is
    (v.y, -v.x, v.z) and the world direction of a local d is (-d.y, d.x, d.z)."""
    m = bbm.Ward(roughness=[0.1, 0.4])
    nrm = np.tile(np.array((0, 0, 1), F)[:, None], (1, N))
    tan = np.tile(np.array((0, 1, 0), F)[:, None], (1, N))
    turn = lambda v: np.stack([v[1], -v[0], v[2]])
    for n in SHAPES:
        for mask in (None, MASK):
            res = seval_call(m, nrm, tan, DOUT, XI, n, mask=mask, shift=shift)
            want = tf.seval_call(m, None, turn(DOUT), XI, n, mask=mask, shift=shift)
            dx, dy = want["dx"], want["dy"]
            want["dx"], want["dy"] = -dy, dx
            for k in SOUTS:
                g, w = res[k], want[k]
                assert ((g == w) | (np.isnan(g) & np.isnan(w))).all(), ("sample_eval", n, k)
            for mode in (1, 2, 3):
                res = eval_call(m, nrm, tan, DIN, DOUT, n, mask=mask, mode=mode, shift=shift)
                want = te.eval_call(m, None, turn(DIN), turn(DOUT), n, mask=mask, mode=mode, shift=shift)
                want["cos"] = np.where(np.ones(n, bool) if mask is None else mask[:n] != 0, DIN[2][:n], F(0))
                for k in res:
                    g, w = res[k], want[k]
                    assert ((g == w) | (np.isnan(g) & np.isnan(w))).all(), ("eval_pdf", n, mode, k)
    # the tangent turns the lobe: upper-hemisphere eval lanes against the normal-only call
    got = eval_call(m, nrm, tan, DIN, DOUT, N, mode=1, cos=False, shift=shift)["r"]
    plain = te.eval_call(m, nrm, DIN, DOUT, N, mode=1, cos=False, shift=shift)["r"]
    up = (DIN[2] > 0) & (DOUT[2] > 0)
    assert up.sum() > 100
    differ = np.abs(got - plain) > 0.01 * np.maximum(np.abs(got), np.abs(plain))
    assert (differ & up).sum() > 0.5 * up.sum(), ((differ & up).sum(), up.sum())


# ------------------------------------------------------------------------ 4. fused equals staged

SEVAL_VARIANTS = [dict(value=True, weight=True), dict(value=False, weight=True)]
EVAL_VARIANTS = [dict(mode=mode, cos=cos) for mode in (1, 2, 3) for cos in (True, False)]
FULL_SHAPES = (257, 1217)


def exact_modes(name):
    return (False, True) if name in te.EXACT_ROWS else (None,)


def fused_is_staged(m, name, material=None):
    kw = {} if material is None else dict(material=material)
    for n in SHAPES:
        for shift in (0, 1):
            full = n in FULL_SHAPES
            for exact in exact_modes(name):
                for j, v in enumerate(SEVAL_VARIANTS):
                    for mask in ((None, MASK) if full else ((MASK, None)[(j + shift) % 2],)):
                        got = seval_call(m, NORMAL, TANGENT, DOUT, XI, n, mask=mask, shift=shift, exact=exact, **v, **kw)
                        want = staged_seval(m, n, mask=mask, shift=shift, exact=exact, **v, **kw)
                        same_results(got, want, (name, "sample_eval", n, shift, exact, v, mask is not None))
                for j, v in enumerate(EVAL_VARIANTS):
                    for mask in ((None, MASK) if full else ((MASK, None)[(j + shift) % 2],)):
                        got = eval_call(m, NORMAL, TANGENT, DIN, DOUT, n, mask=mask, shift=shift, exact=exact, **v, **kw)
                        want = staged_eval(m, n, mask=mask, shift=shift, exact=exact, **v, **kw)
                        same_results(got, want, (name, "eval_pdf", n, shift, exact, v, mask is not None))


@pytest.mark.parametrize("name", ANISOTROPIC)
def test_fused_is_staged(bbm, merl, name):
    fused_is_staged(tf.instance(bbm, merl, name), name)


@pytest.mark.parametrize("name", ANISOTROPIC)
def test_fused_is_staged_table(bbm, name):
    t = bbm.MaterialTable(name, te.three_materials(name))
    fused_is_staged(t, name, material=MATERIAL)
    t.close()


def test_the_tangent_is_read(bbm):
    """On the anisotropic rows the tangent call is not the normal-only call (the other half of test 5)."""
    for name in ANISOTROPIC:
        m = tf.instance(bbm, None, name)
        p = m.parameter_values().astype(F)
        if name in ("Ward", "WardDuer", "WardDuerGeislerMoroder"):
            p[3:5] = (0.1, 0.4)
            m.set_parameter_values(p)
        got = eval_call(m, NORMAL, TANGENT, DIN, DOUT, N, mode=3, cos=False)
        plain = te.eval_call(m, NORMAL, DIN, DOUT, N, mode=3, cos=False)
        if any((got[k] != plain[k]).any() for k in ("r", "pdf")):
            continue
        # equal x and y parameters: an isotropic lobe, whatever the frame -- but then the sampled direction turns
        s = seval_call(m, NORMAL, TANGENT, DOUT, XI, N)
        sp = tf.seval_call(m, NORMAL, DOUT, XI, N)
        assert (s["dx"] != sp["dx"]).any(), name


# ------------------------------------------------------------------------ 5. the other rows ignore the tangent

@pytest.mark.parametrize("name", ISOTROPIC)
def test_isotropic_rows_ignore_the_tangent(bbm, merl, name):
    n = 257
    m = tf.instance(bbm, merl, name)
    for shift in (0, 1):
        same_results(seval_call(m, NORMAL, TANGENT, DOUT, XI, n, mask=MASK, shift=shift),
                     tf.seval_call(m, NORMAL, DOUT, XI, n, mask=MASK, shift=shift), (name, "sample_eval", shift))
        same_results(eval_call(m, NORMAL, TANGENT, DIN, DOUT, n, mask=MASK, shift=shift),
                     te.eval_call(m, NORMAL, DIN, DOUT, n, mask=MASK, shift=shift), (name, "eval_pdf", shift))


@pytest.mark.parametrize("name", ISOTROPIC_TABLES)
def test_isotropic_tables_ignore_the_tangent(bbm, name):
    n = 257
    t = bbm.MaterialTable(name, te.three_materials(name))
    for shift in (0, 1):
        same_results(seval_call(t, NORMAL, TANGENT, DOUT, XI, n, mask=MASK, shift=shift, material=MATERIAL),
                     tf.seval_call(t, NORMAL, DOUT, XI, n, mask=MASK, shift=shift, material=MATERIAL),
                     (name, "sample_eval", shift))
        same_results(eval_call(t, NORMAL, TANGENT, DIN, DOUT, n, mask=MASK, shift=shift, material=MATERIAL),
                     te.eval_call(t, NORMAL, DIN, DOUT, n, mask=MASK, shift=shift, material=MATERIAL),
                     (name, "eval_pdf", shift))
    t.close()


# ------------------------------------------------------------------------ 6. sets

SET_ROWS = ["Ward", "GGX", "GGXHeitz", "Lambertian"]


def set_call(kind, plan, normal, tangent, n, mask, shift, **kw):
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], **tins(tangent, n)}
    if kind == "eval":
        ins.update({"ix": DIN[0][:n], "iy": DIN[1][:n], "iz": DIN[2][:n], "ox": DOUT[0][:n], "oy": DOUT[1][:n], "oz": DOUT[2][:n]})
        outs, order = EOUTS, ("ix", "iy", "iz", "ox", "oy", "oz")
    else:
        ins.update({"ox": DOUT[0][:n], "oy": DOUT[1][:n], "oz": DOUT[2][:n], "xi0": XI[0][:n], "xi1": XI[1][:n]})
        outs, order = SOUTS, ("ox", "oy", "oz", "xi0", "xi1")
    if mask is not None:
        ins["mask"] = mask[:n]
    a = Arena(n, shift, ins, outs)
    fn = lib.bbm_hip_set_eval_pdf_tangent if kind == "eval" else lib.bbm_hip_set_sample_eval_tangent
    bbm_amd._lib.check(fn(plan._live(), 0, *(a.ptr(k) for k in ("nx", "ny", "nz")), *tptrs(a, tangent),
                          *(a.ptr(k) for k in order), a.ptr("mask") if mask is not None else None, n, 3, 0,
                          *(a.ptr(k) for k in outs), stream()))
    return a.results()


@pytest.mark.parametrize("shift", [0, 1])
def test_sets(bbm, shift):
    tables = [bbm.MaterialTable(name, te.three_materials(name)) for name in SET_ROWS]
    mset = bbm.MaterialSet(tables)
    rng = np.random.default_rng(SEED + 1)
    ids = rng.integers(0, 12, N).astype(np.int64)
    ids[[13, 270]] = 12                                   # past the total
    ids[[14, 271]] = -1
    ids = ids.astype(np.uint32)
    try:
        for n in SHAPES:
            gid = torch.from_numpy(ids[:n].astype(np.int32)).cuda()
            plan = mset.plan(gid)
            if True:
                for mask in (None, MASK):
                    got_e = set_call("eval", plan, NORMAL, TANGENT, n, mask, shift)
                    got_s = set_call("seval", plan, NORMAL, TANGENT, n, mask, shift)
                    for k, t in enumerate(tables):
                        mine = (ids[:n] >= 3 * k) & (ids[:n] < 3 * k + 3)
                        if k == 0:
                            mine |= ids[:n] >= 12                # an id past the total is row 0's masked-index lane
                        if not mine.any():
                            continue
                        local = np.where(ids[:n] >= 12, np.uint32(0xFFFFFFFF), ids[:n] - np.uint32(3 * k)).astype(np.uint32)
                        want_e = eval_call(t, NORMAL, TANGENT, DIN, DOUT, n, mask=mask, shift=shift, material=local)
                        want_s = seval_call(t, NORMAL, TANGENT, DOUT, XI, n, mask=mask, shift=shift, material=local)
                        for key in EOUTS:
                            same_bits(got_e[key][mine], want_e[key][mine], ("set eval_pdf", n, SET_ROWS[k], key))
                        for key in SOUTS:
                            same_bits(got_s[key][mine], want_s[key][mine], ("set sample_eval", n, SET_ROWS[k], key))
                    # three NULL tangent pointers: the normal-only set call
                    same_results(set_call("eval", plan, NORMAL, None, n, mask, shift),
                                 {k: v for k, v in zip(EOUTS, _set_plain_eval(plan, n, mask, shift))}, ("set null", n))
            plan.close()
    finally:
        mset.close()
        for t in tables:
            t.close()


def _set_plain_eval(plan, n, mask, shift):
    lib = bbm_amd._lib.load()
    ins = {"nx": NORMAL[0][:n], "ny": NORMAL[1][:n], "nz": NORMAL[2][:n], "ix": DIN[0][:n], "iy": DIN[1][:n],
           "iz": DIN[2][:n], "ox": DOUT[0][:n], "oy": DOUT[1][:n], "oz": DOUT[2][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    a = Arena(n, shift, ins, EOUTS)
    bbm_amd._lib.check(lib.bbm_hip_set_eval_pdf(
        plan._live(), 0, *(a.ptr(k) for k in ("nx", "ny", "nz", "ix", "iy", "iz", "ox", "oy", "oz")),
        a.ptr("mask") if mask is not None else None, n, 3, 0, *(a.ptr(k) for k in EOUTS), stream()))
    r = a.results()
    return [r[k] for k in EOUTS]


# ------------------------------------------------------------------------ 7. the Python surface

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_python_surface(bbm):
    n = 257
    nrm, tan, din, dout, xi, mask = (dev(a[..., :n]) for a in (NORMAL, TANGENT, DIN, DOUT, XI, MASK))
    m = bbm.Ward(roughness=[0.1, 0.4])
    # frames
    for to_local, fn in ((True, bbm.to_local), (False, bbm.to_global)):
        got = fn(nrm, dev(VEC[:, :n]), mask, tangent=tan).cpu().numpy()
        same_bits(got, frame_call(to_local, NORMAL, TANGENT, VEC, n, MASK), ("to_local" if to_local else "to_global"))
    # a model
    rgb, pdf, cos = m.eval_pdf(din, dout, mask=mask, normal=nrm, tangent=tan, cosine=True)
    want = eval_call(m, NORMAL, TANGENT, DIN, DOUT, n, mask=MASK)
    same_bits(rgb.cpu().numpy(), np.stack([want["r"], want["g"], want["b"]]), "model rgb")
    same_bits(pdf.cpu().numpy(), want["pdf"], "model pdf")
    same_bits(cos.cpu().numpy(), want["cos"], "model cos")
    same_bits(m.eval(din, dout, mask=mask, normal=nrm, tangent=tan).cpu().numpy()[0], want["r"], "model eval")
    same_bits(m.pdf(din, dout, mask=mask, normal=nrm, tangent=tan).cpu().numpy(), want["pdf"], "model pdf()")
    s, v, w = m.sample_eval(dout, xi, mask=mask, normal=nrm, tangent=tan)
    wants = seval_call(m, NORMAL, TANGENT, DOUT, XI, n, mask=MASK)
    same_bits(s.direction.cpu().numpy(), np.stack([wants["dx"], wants["dy"], wants["dz"]]), "model dir")
    same_bits(v.cpu().numpy()[0], wants["r"], "model value")
    same_bits(w.cpu().numpy()[2], wants["wb"], "model weight")
    # a table
    mat = dev(MATERIAL[:n].astype(np.int32))
    t = bbm.MaterialTable("Ward", te.three_materials("Ward"))
    if True:
        rgb, pdf = t.eval_pdf(din, dout, mask=mask, material=mat, normal=nrm, tangent=tan)
        want = eval_call(t, NORMAL, TANGENT, DIN, DOUT, n, mask=MASK, material=MATERIAL, cos=False)
        same_bits(rgb.cpu().numpy()[1], want["g"], "table g")
        same_bits(pdf.cpu().numpy(), want["pdf"], "table pdf")
        s, v, w = t.sample_eval(dout, xi, mask=mask, material=mat, normal=nrm, tangent=tan)
        wants = seval_call(t, NORMAL, TANGENT, DOUT, XI, n, mask=MASK, material=MATERIAL)
        same_bits(s.direction.cpu().numpy()[0], wants["dx"], "table dir")
        same_bits(w.cpu().numpy()[0], wants["wr"], "table weight")
        # a set of that one table: lane i is the table call's lane
        mset = bbm.MaterialSet([t])
        rgb, pdf = mset.eval_pdf(din, dout, mask=mask, material=mat, normal=nrm, tangent=tan)
        same_bits(rgb.cpu().numpy()[1], want["g"], "set g")
        s, v, w = mset.sample_eval(dout, xi, mask=mask, material=mat, normal=nrm, tangent=tan)
        same_bits(s.direction.cpu().numpy()[0], wants["dx"], "set dir")
        mset.close()
        t.close()


@pytest.mark.parametrize("runtime", [False, True])
def test_aggregate_model_is_staged(bbm, runtime):
    """Aggregate(Lambertian(), Ward()) has an anisotropic child: tangent= goes to the frame calls around the tree's own
    local calls."""
    n = 257
    nrm, tan, din, dout, xi, mask = (dev(a[..., :n]) for a in (NORMAL, TANGENT, DIN, DOUT, XI, MASK))
    tree = bbm.Aggregate(bbm.Lambertian(), bbm.Ward(roughness=[0.1, 0.4]), fused=False, runtime=runtime)
    assert isinstance(tree, bbm.AggregateModel)
    rgb, pdf, cos = tree.eval_pdf(din, dout, mask=mask, normal=nrm, tangent=tan, cosine=True)
    li, lo = bbm.to_local(nrm, din, mask, tangent=tan), bbm.to_local(nrm, dout, mask, tangent=tan)
    wrgb, wpdf = tree.eval_pdf(li, lo, mask=mask)
    same_bits(rgb.cpu().numpy(), wrgb.cpu().numpy(), "tree rgb")
    same_bits(pdf.cpu().numpy(), wpdf.cpu().numpy(), "tree pdf")
    same_bits(cos.cpu().numpy(), li[2].cpu().numpy(), "tree cos")
    s, v, w = tree.sample_eval(dout, xi, mask=mask, normal=nrm, tangent=tan)
    ws, wv, ww = tree.sample_eval(lo, xi, mask=mask)
    same_bits(s.direction.cpu().numpy(), bbm.to_global(nrm, ws.direction, mask, tangent=tan).cpu().numpy(), "tree dir")
    same_bits(v.cpu().numpy(), wv.cpu().numpy(), "tree value")
    same_bits(w.cpu().numpy(), ww.cpu().numpy(), "tree weight")
    # and the tangent matters to the tree
    plain = tree.eval_pdf(din, dout, mask=mask, normal=nrm)[0]
    assert (plain != rgb).any()
