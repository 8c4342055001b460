"""eval / pdf / eval + pdf in world space on the GPU (bbm_amd/csrc/eval_world.hpp, k_eval_pdf_compact<FRAME>, the per-lane
kernels of lanes.hpp over EvalTabWorldArgs): bbm_hip_eval_pdf_world / bbm_hip_eval_pdf_table_world and the Python
`normal=` / `cosine=` surface of eval_pdf, eval and pdf.

What is held, and to what:
  1. fused equals staged -- frame_to_local(normal, in), frame_to_local(normal, out), the local call -- bit for bit on
     every output array, all 49 rows and the 43 table rows; the cosine is the z of the first call;
  2. the same over the shape list, and for He over the compaction tile and its edges;
  3. the identity frame: every normal (0, 0, 1) makes the world call the local call (`==`: -0 equals 0), cosine in_z;
  4. a lane whose normal is not live is that lane with mask == 0;
  5. compaction sees the local directions: under normals (0, 0, -1) the world upper hemisphere is all dead;
  6. the Python surface returns the C-ABI results.
"Bit for bit" = equal int32 views; NaN lanes compare by where they are NaN.

Every C-ABI call takes its arrays, inputs included, out of one sentinel-filled allocation, 16-byte aligned (the quad
kernels and their scalar tail, the compaction kernel) or 4 bytes further (the one-lane kernels); whatever lies outside
the call's output arrays must be unchanged afterwards.

The normals (1217 lanes) are tests/test_gpu_frame.py's: random unit vectors, with (0, 0, 1), (0, 0, -1), (0, 0, 0),
(1, 0, 0), z = -0.0, a normal of length 1e-3 and one of length 1e3 in the first eight lanes, and a second (0, 0, 0) on
lane 256, the scalar tail of n = 257.  The directions: an even lane draws local upper-hemisphere directions and takes
them to world space through a float64 restatement of the frame, an odd lane draws over the whole sphere; so at least
40 % of the lanes have both local z > 0.01 (the models' live region, the compaction kernel's live pairs) and at least
10 % have one below the horizon (asserted on the CPU at import, by the float64 restatement).

Parameters: each row's golden sets, the first and the last (for Ribardiere and Bagher the last that gives finite
values, LAST_FINITE_SET); a table holds those two and the first scaled by 0.9.
"""
import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou
from tests.test_gpu_loss_models import LAST_FINITE_SET

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(np.finfo(np.float32).eps)
N = 1217
SEED = 0xE7A1F
NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
UNSUPPORTED = ["He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"]
SUPPORTED = [n for n in NAMES if n not in UNSUPPORTED]
SHAPES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1217]
SHAPE_ROWS = ["Lambertian", "CookTorrance", "Aggregate<Lambertian,Bagher>"]
TILE_SHAPES = [1023, 1024, 1025]          # k_eval_pdf_compact's tile of 4 x 256 pairs and its edges
SENTINEL = F(-12345.678)
GUARD = 4
OUTS = ["r", "g", "b", "pdf", "cos"]
# the rows with an exact-mode eval kernel of their own (model_has_exact: the Beckmann, Student-T and Low NDFs, Bagher,
# LowSmooth, and the aggregates over them); both modes are run on them
EXACT_ROWS = ["CookTorrance", "LowCookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "NganCookTorrance",
              "Ribardiere", "RibardiereAnisotropic", "LowMicrofacet", "LowMicrofacetFit", "LowSmooth", "Bagher",
              "Aggregate<Lambertian,Bagher>", "Aggregate<Lambertian,CookTorrance>",
              "Aggregate<Lambertian,LowCookTorrance>", "Aggregate<Lambertian,NganCookTorrance>",
              "Aggregate<Lambertian,LowMicrofacetFit>", "Aggregate<Lambertian,LowSmooth>"]
AGGREGATE = "Aggregate<Lambertian,CookTorrance>"


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


# ------------------------------------------------------------------------ the arena (tests/test_gpu_frame.py's)

class Arena:
    """Named arrays of n 4-byte elements (or n bytes: the mask) in one sentinel-filled float32 allocation, each GUARD
    floats after a 16-byte boundary plus `shift` floats.  ins: name -> numpy array; outs: names."""

    def __init__(self, n, shift, ins, outs):
        self.n, self.outs = n, list(outs)
        names = list(ins) + self.outs
        stride = (GUARD + n + 1 + GUARD + 3) // 4 * 4
        self.first = {k: j * stride + GUARD + shift for j, k in enumerate(names)}
        host = np.full(len(names) * stride, SENTINEL, F)
        for k, a in ins.items():
            a = np.ascontiguousarray(a)
            assert a.shape == (n,), (k, a.shape)
            if a.dtype == np.uint8:
                host.view(np.uint8)[4 * self.first[k]:4 * self.first[k] + n] = a
            else:
                assert a.dtype.itemsize == 4, k
                host[self.first[k]:self.first[k] + n] = a.view(F)
        self.before = host
        self.dev = torch.from_numpy(host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        for k in names:
            assert (self.ptr(k) % 16 == 0) == (shift == 0)

    def ptr(self, k):
        return self.dev.data_ptr() + 4 * self.first[k]

    def results(self, given=None):
        """name -> (n,) float32 array of the outputs, after checking that nothing else was written."""
        host = self.dev.cpu().numpy()
        touched = np.zeros(host.size, bool)
        res = {}
        for k in self.outs:
            if given is None or given[k]:
                touched[self.first[k]:self.first[k] + self.n] = True
                res[k] = host[self.first[k]:self.first[k] + self.n].copy()
        bad = np.nonzero((host.view(np.int32) != self.before.view(np.int32)) & ~touched)[0]
        assert bad.size == 0, f"{bad.size} floats outside the call's outputs written, first at {bad[:8]}"
        return res


def stream():
    return torch.cuda.current_stream().cuda_stream


def frame_call(normal, v, n, mask=None, shift=0):
    """bbm_hip_frame_to_local on the first n lanes of (3, >= n) numpy arrays -> (3, n)."""
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], "x": v[0][:n], "y": v[1][:n], "z": v[2][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    a = Arena(n, shift, ins, ["rx", "ry", "rz"])
    bbm_amd._lib.check(lib.bbm_hip_frame_to_local(*(a.ptr(k) for k in ("nx", "ny", "nz", "x", "y", "z")),
                                                  a.ptr("mask") if mask is not None else None, n, a.ptr("rx"),
                                                  a.ptr("ry"), a.ptr("rz"), stream()))
    r = a.results()
    return np.stack([r["rx"], r["ry"], r["rz"]])


def eval_call(m, normal, din, dout, n, comp=3, mask=None, mode=3, cos=True, shift=0, exact=None, material=None):
    """bbm_hip_eval_pdf(_table) (normal None; the uniform call through the entry point of its mode) or
    bbm_hip_eval_pdf(_table)_world on the first n lanes.  mode: 1 eval, 2 pdf, 3 both."""
    lib = bbm_amd._lib.load()
    ins = {}
    if normal is not None:
        ins.update({"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n]})
    ins.update({"ix": din[0][:n], "iy": din[1][:n], "iz": din[2][:n], "ox": dout[0][:n], "oy": dout[1][:n], "oz": dout[2][:n]})
    if mask is not None:
        ins["mask"] = mask[:n]
    if material is not None:
        ins["material"] = material[:n]
    given = {"r": bool(mode & 1), "g": bool(mode & 1), "b": bool(mode & 1), "pdf": bool(mode & 2),
             "cos": cos and normal is not None}
    a = Arena(n, shift, ins, OUTS)
    pre = [a.ptr(k) for k in ("nx", "ny", "nz")] if normal is not None else []
    dirs = [a.ptr(k) for k in ("ix", "iy", "iz", "ox", "oy", "oz")]
    mid = [a.ptr("mask") if mask is not None else None, n, comp, 0]
    outs = [a.ptr(k) if given[k] else None for k in ("r", "g", "b", "pdf")]
    tail = ([a.ptr("cos") if given["cos"] else None] if normal is not None else []) + [stream()]
    if material is not None:
        fn = lib.bbm_hip_eval_pdf_table if normal is None else lib.bbm_hip_eval_pdf_table_world
        rc = fn(m._live(), m._flags(exact), a.ptr("material"), *pre, *dirs, *mid, *outs, *tail)
    elif normal is not None:
        rc = lib.bbm_hip_eval_pdf_world(m._call_id(exact), m._pptr(), m._params.size, *pre, *dirs, *mid, *outs, *tail)
    else:
        head = (m._call_id(exact), m._pptr(), m._params.size)
        if mode == 3:
            rc = lib.bbm_hip_eval_pdf(*head, *dirs, *mid, *outs, *tail)
        elif mode == 1:
            rc = lib.bbm_hip_eval(*head, *dirs, *mid, *outs[:3], *tail)
        else:
            rc = lib.bbm_hip_pdf(*head, *dirs, *mid, outs[3], *tail)
    bbm_amd._lib.check(rc)
    return a.results(given)


def live_lanes(normal):
    """|n|^2 > epsilon in the kernel's float32 order."""
    x, y, z = (normal[k].astype(F) for k in range(3))
    with np.errstate(all="ignore"):
        nn = ((F(0) + x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)
    return nn.astype(F) > EPS


def staged(m, normal, din, dout, n, mask=None, shift=0, cos=True, **kw):
    """frame_to_local on `in`, frame_to_local on `out`, the local call, every one through the C-ABI with the same mask:
    the caller's with the lanes of a normal that is not live cleared (the contract: such a lane is a masked lane of
    the pipeline).  The cosine is the first call's z."""
    mk = (np.ones(n, np.uint8) if mask is None else mask[:n].copy())
    mk[~live_lanes(normal)[:n]] = 0
    li = frame_call(normal, din, n, mk, shift)
    lo = frame_call(normal, dout, n, mk, shift)
    res = eval_call(m, None, li, lo, n, mask=mk, shift=shift, **kw)
    if cos:
        res["cos"] = li[2]
    return res


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    nan = np.isnan(g)
    assert (nan == np.isnan(w)).all(), (what, "NaN lanes differ", np.nonzero(nan != np.isnan(w))[0][:8])
    g, w = np.where(nan, F(0), g), np.where(nan, F(0), w)
    diff = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
    assert diff.size == 0, (what, f"{diff.size} lanes differ", diff[:8], g[diff[:4]], w[diff[:4]])


def same_results(res, want, what):
    assert set(res) == set(want), (what, sorted(res), sorted(want))
    for k in res:
        same_bits(res[k], want[k], (what, k))


# ------------------------------------------------------------------------ shared inputs (computed once, never written)

def make_normals(rng, n):
    """tests/test_gpu_frame.py's NORMALS recipe."""
    v = rng.standard_normal((3, n))
    v = (v / np.linalg.norm(v, axis=0)).astype(F)
    v[:, 0] = (0, 0, 1)
    v[:, 1] = (0, 0, -1)
    v[:, 2] = (0, 0, 0)
    v[:, 3] = (1, 0, 0)
    v[:, 4] = (0.6, 0.8, -0.0)
    v[:, 5] *= F(1e-3)
    v[:, 6] *= F(1e3)
    v[:, 256] = (0, 0, 0)
    v[:, 300:340] *= F(1e-3)
    v[:, 340:380] *= F(1e3)
    v[:, 400] = (0.0, -1.0, -0.0)
    v[:, 401] = (0, 0, 1)
    v[:, 402] = (0, 0, -1)
    assert np.signbit(v[2, 4]) and np.signbit(v[2, 400])
    return v


def frame64(normal):
    """core/shading_frame.h:26-58 in float64: the columns X, Y, Z of toGlobalShadingFrame(normal)."""
    n = normal.astype(np.float64)
    with np.errstate(all="ignore"):
        Z = n / np.sqrt((n * n).sum(0))
        sign = np.copysign(1.0, Z[2])
        a = -1.0 / (sign + Z[2])
        b = Z[0] * Z[1] * a
        X = np.stack([1.0 + sign * Z[0] * Z[0] * a, sign * b, -sign * Z[0]])
        Y = np.stack([b, sign + Z[1] * Z[1] * a, -Z[1]])
    return X, Y, Z


def local_z64(normal, v):
    return (frame64(normal)[2] * v.astype(np.float64)).sum(0)


def make_direction(rng, normal):
    """Even lanes: a local upper-hemisphere direction (z >= 0.02) taken to world space by the float64 frame; odd lanes
    (and the lanes without a frame): uniform over the sphere."""
    n = normal.shape[1]
    sphere = rng.standard_normal((3, n))
    sphere /= np.linalg.norm(sphere, axis=0)
    z = rng.uniform(0.02, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - z * z)
    local = np.stack([s * np.cos(phi), s * np.sin(phi), z])
    X, Y, Z = frame64(normal)
    world = X * local[0] + Y * local[1] + Z * local[2]
    use = (np.arange(n) % 2 == 0) & np.isfinite(world).all(0)
    return np.where(use, world, sphere).astype(F)


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    normal = make_normals(rng, N)
    din, dout = make_direction(rng, normal), make_direction(rng, normal)
    return rng, normal, din, dout


def guard(normal, din, dout):
    """By the float64 restatement: the share of lanes with both local z > 0.01, and with one of them < 0."""
    with np.errstate(all="ignore"):
        zi, zo = local_z64(normal, din), local_z64(normal, dout)
    return ((zi > 0.01) & (zo > 0.01)).mean(), ((zi < 0) | (zo < 0)).mean()


_RNG, NORMAL, DIN, DOUT = make_inputs(SEED)
_BOTH_UP, _ONE_DOWN = guard(NORMAL, DIN, DOUT)
assert _BOTH_UP >= 0.40 and _ONE_DOWN >= 0.10, (_BOTH_UP, _ONE_DOWN)
MASK = np.ones(N, np.uint8)
MASK[[9, 10, 254, N - 1]] = 0
MATERIAL = _RNG.integers(0, 3, N).astype(np.int64)
MATERIAL[[11, 257]] = -1                                   # out of range: the component is switched off
MATERIAL[[12, 258]] = 3
MATERIAL = MATERIAL.astype(np.uint32)
for _a in (NORMAL, DIN, DOUT, MASK, MATERIAL):
    _a.flags.writeable = False


@pytest.fixture(scope="module")
def merl(bbm, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("merl") / "synthetic.binary")
    ou.synthetic_merl(path)
    return bbm.Merl(path)


def golden_sets(name):
    """The row's first and last golden parameter sets (the last finite one for the rows LAST_FINITE_SET names)."""
    if name not in META:
        return []
    g = ou.golden_model(name)
    last = LAST_FINITE_SET.get(name, len(META[name]["sets"]) - 1)
    return [g["params0"].astype(F)] + ([g[f"params{last}"].astype(F)] if last > 0 else [])


def instances(bbm, merl, name):
    """One model per golden set of the row (Merl: the synthetic table)."""
    if name == "Merl":
        return [merl]
    out = []
    for p in golden_sets(name) or [None]:
        m = bbm.BsdfModel(name)
        if p is not None:
            m.set_parameter_values(p)
        out.append(m)
    return out


def three_materials(name):
    sets = golden_sets(name)
    m = bbm_amd.BsdfModel(name)
    base = sets[0] if sets else m.parameter_values().astype(F)
    scaled = np.clip(base * F(0.9), m.parameter_lower_bound(), m.parameter_upper_bound()).astype(F)
    return np.stack([base, sets[-1] if sets else base, scaled])


def test_rows_are_listed(bbm):
    lib = bbm._lib.load()
    assert len(NAMES) == 49 and len(SUPPORTED) == 43
    assert [n for i, n in enumerate(NAMES) if lib.bbm_hip_model_has_table(i) == 1] == SUPPORTED
    assert set(SHAPE_ROWS + EXACT_ROWS + [AGGREGATE, "He"]) <= set(NAMES)
    assert (~live_lanes(NORMAL)).sum() == 2 and MASK[2] == 1 and MASK[256] == 1
    assert (MATERIAL >= 3).sum() == 4


# ------------------------------------------------------------------------ 1. fused equals staged

# the three modes, mask on / off, the cosine on / off, aligned (the quad and compaction kernels) and not (one lane)
CASES = [dict(mode=3, mask=True, cos=True, shift=0), dict(mode=3, mask=False, cos=False, shift=0),
         dict(mode=1, mask=True, cos=False, shift=0), dict(mode=2, mask=False, cos=True, shift=0),
         dict(mode=3, mask=True, cos=True, shift=1), dict(mode=1, mask=False, cos=True, shift=1),
         dict(mode=2, mask=True, cos=False, shift=1), dict(mode=3, mask=False, cos=False, shift=1)]


def fused_is_staged(m, n, what, material=None, cases=CASES, modes=(None,), comp=3):
    got = None
    for exact in modes:
        for c in cases:
            mask = MASK if c["mask"] else None
            kw = dict(mode=c["mode"], cos=c["cos"], exact=exact, material=material, comp=comp)
            got = eval_call(m, NORMAL, DIN, DOUT, n, mask=mask, shift=c["shift"], **kw)
            want = staged(m, NORMAL, DIN, DOUT, n, mask=mask, shift=c["shift"], **kw)
            same_results(got, want, (what, n, exact, tuple(c.items())))
            if c["mode"] & 1 and material is None:
                # not zeros against zeros.  Every row can meet this at n >= 63: each is nonzero somewhere in the upper
                # hemisphere (Merl's synthetic table is positive there), where 40 % of the lanes lie; the first
                # lanes hold the special normals, so the shortest shapes are not asked.
                assert n < 63 or (want["r"] != 0).any(), (what, "the staged r is zero on every lane")
    return got


def exact_modes(name):
    return (False, True) if name in EXACT_ROWS else (None,)


@pytest.mark.parametrize("name", NAMES)
def test_fused_is_staged(bbm, merl, name):
    for m in instances(bbm, merl, name):
        got = fused_is_staged(m, N, name, modes=exact_modes(name))
    # the last case stores no cosine; the one before the last of the aligned ones does: the dead lanes' is +0
    got = eval_call(m, NORMAL, DIN, DOUT, N, mask=MASK)
    for lane in (2, 9, 256):
        assert got["cos"].view(np.int32)[lane] == 0, lane


@pytest.mark.parametrize("name", SUPPORTED)
def test_fused_is_staged_table(bbm, name):
    table = bbm.MaterialTable(name, three_materials(name))
    assert len(table) == 3 and MATERIAL[11] == 0xffffffff
    fused_is_staged(table, N, name, material=MATERIAL, modes=exact_modes(name))
    # a lane whose material is out of range: the component is off, the cosine is still the transformed z
    got = eval_call(table, NORMAL, DIN, DOUT, N, material=MATERIAL)
    want = frame_call(NORMAL, DIN, N)[2]
    for lane in (11, 12, 257, 258):
        assert got["cos"].view(np.int32)[lane] == want.view(np.int32)[lane] and want[lane] != 0, lane
    table.close()


@pytest.mark.parametrize("comp", [1, 2])
def test_fused_is_staged_components(bbm, comp):
    m = bbm.BsdfModel(AGGREGATE)
    m.set_parameter_values(golden_sets(AGGREGATE)[0])
    fused_is_staged(m, N, (AGGREGATE, comp), comp=comp)
    table = bbm.MaterialTable(AGGREGATE, three_materials(AGGREGATE))
    fused_is_staged(table, N, (AGGREGATE, comp, "table"), material=MATERIAL, comp=comp)
    table.close()


def test_fused_is_staged_runtime_aggregate(bbm):
    m = bbm.Aggregate(bbm.Lambertian(albedo=[0.2, 0.5, 0.8]), bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2,
                                                                                 eta=1.5), runtime=True)
    assert isinstance(m, bbm.BsdfModel) and m.runtime and m.name == AGGREGATE
    for comp in (3, 1, 2):
        fused_is_staged(m, N, ("runtime", comp), comp=comp)


# ------------------------------------------------------------------------ 2. shapes

SHAPE_CASES = [dict(mode=3, mask=True, cos=True, shift=0), dict(mode=3, mask=True, cos=True, shift=1)]


@pytest.mark.parametrize("name", SHAPE_ROWS)
def test_fused_is_staged_shapes(bbm, merl, name):
    m = instances(bbm, merl, name)[0]
    table = bbm.MaterialTable(name, three_materials(name))
    for n in SHAPES:
        fused_is_staged(m, n, name, cases=SHAPE_CASES)
        fused_is_staged(table, n, name, material=MATERIAL, cases=SHAPE_CASES)
    table.close()


def test_fused_is_staged_shapes_compaction_tile(bbm, merl):
    m = instances(bbm, merl, "He")[0]
    for n in SHAPES + TILE_SHAPES:
        fused_is_staged(m, n, "He", cases=SHAPE_CASES)


# ------------------------------------------------------------------------ 3. the identity frame

def identity_case(m, n, material=None, modes=(None,)):
    up = np.zeros((3, N), F)
    up[2] = 1
    for exact in modes:
        for shift in (0, 1):
            world = eval_call(m, up, DIN, DOUT, n, exact=exact, material=material, shift=shift)
            local = eval_call(m, None, DIN, DOUT, n, exact=exact, material=material, shift=shift)
            for k in ("r", "g", "b", "pdf"):
                g, w = world[k], local[k]
                nan = np.isnan(g)
                assert (nan == np.isnan(w)).all(), (k, exact, shift)
                bad = np.nonzero(g[~nan] != w[~nan])[0]
                assert bad.size == 0, (k, exact, shift, bad[:8], g[~nan][bad[:4]], w[~nan][bad[:4]])
            assert (world["cos"] == DIN[2][:n]).all()


@pytest.mark.parametrize("name", NAMES)
def test_identity_frame(bbm, merl, name):
    identity_case(instances(bbm, merl, name)[0], 257, modes=exact_modes(name))


@pytest.mark.parametrize("name", SUPPORTED)
def test_identity_frame_table(bbm, name):
    table = bbm.MaterialTable(name, three_materials(name))
    identity_case(table, 257, material=MATERIAL)
    table.close()


# ------------------------------------------------------------------------ 4. a degenerate lane is a masked lane

@pytest.mark.parametrize("name", ["CookTorrance", "He"])
@pytest.mark.parametrize("shift", [0, 1])
def test_degenerate_lane_is_a_masked_lane(bbm, merl, name, shift):
    """A (0, 0, 0) or NaN normal with mask 1 gives what the same lane gives with a live normal and mask 0."""
    m = instances(bbm, merl, name)[0]
    n = 257
    nrm = NORMAL.copy()
    nrm[:, 20] = (np.nan, 0.0, 1.0)
    nrm[:, 21] = (0.0, 1e-5, 0.0)                        # |n|^2 = 1e-10 <= epsilon
    a = eval_call(m, nrm, DIN, DOUT, n, mask=MASK, shift=shift)
    dead = [2, 20, 21, 256]
    assert not live_lanes(nrm)[dead].any() and MASK[dead].all()
    nrm2 = nrm.copy()
    for lane in dead:
        nrm2[:, lane] = (0.0, 0.6, 0.8)
    mask = MASK.copy()
    mask[dead] = 0
    b = eval_call(m, nrm2, DIN, DOUT, n, mask=mask, shift=shift)
    same_results(a, b, ("degenerate == masked", name))
    assert (a["cos"].view(np.int32)[dead] == 0).all()


# ------------------------------------------------------------------------ 5. compaction sees the local directions

def test_compaction_sees_local_directions(bbm, merl):
    m = instances(bbm, merl, "He")[0]
    rng = np.random.default_rng(SEED + 1)
    z = rng.uniform(0.05, 1.0, (2, N))
    phi = rng.uniform(0.0, 2.0 * np.pi, (2, N))
    s = np.sqrt(1.0 - z * z)
    din = np.stack([s[0] * np.cos(phi[0]), s[0] * np.sin(phi[0]), z[0]]).astype(F)      # the world upper hemisphere
    dout = np.stack([s[1] * np.cos(phi[1]), s[1] * np.sin(phi[1]), z[1]]).astype(F)
    down, up = np.zeros((3, N), F), np.zeros((3, N), F)
    down[2], up[2] = -1, 1
    got = eval_call(m, down, din, dout, N)
    want = {k: v for k, v in staged(m, down, din, dout, N).items()}
    same_results(got, want, "He, normals down")
    for k in ("r", "g", "b", "pdf"):
        assert (want[k] == 0).all() and (got[k].view(np.int32) == 0).all(), k
    assert (got["cos"] < 0).all()
    got = eval_call(m, up, din, dout, N)
    local = eval_call(m, None, din, dout, N)
    for k in ("r", "g", "b", "pdf"):
        same_bits(got[k], local[k], ("He, normals up", k))
    assert (local["r"] != 0).sum() > N // 2 and (local["pdf"] != 0).sum() > N // 2


# ------------------------------------------------------------------------ 6. the Python surface

def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def test_python_surface(bbm, merl):
    nrm, din, dout, mask = dev(NORMAL), dev(DIN), dev(DOUT), dev(MASK)
    ids = dev(MATERIAL.view(np.int32))
    ct = instances(bbm, merl, "CookTorrance")[0]
    table = bbm.MaterialTable("CookTorrance", three_materials("CookTorrance"))
    for exact in (None, True):
        want = eval_call(ct, NORMAL, DIN, DOUT, N, mask=MASK, exact=exact)
        rgb, pdf, cos = ct.eval_pdf(din, dout, mask=mask, normal=nrm, cosine=True, exact=exact)
        assert rgb.shape == (3, N) and pdf.shape == (N,) and cos.shape == (N,) and cos.dtype == torch.float32
        got = {"r": rgb[0], "g": rgb[1], "b": rgb[2], "pdf": pdf, "cos": cos}
        same_results({k: v.cpu().numpy() for k, v in got.items()}, want, ("eval_pdf", exact))
        res = ct.eval_pdf(din, dout, mask=mask, normal=nrm, exact=exact)
        assert len(res) == 2
        same_bits(res[1].cpu().numpy(), want["pdf"], "eval_pdf, no cosine")
        rgb = ct.eval(din, dout, mask=mask, normal=nrm, exact=exact)
        for j, k in enumerate("rgb"):
            same_bits(rgb[j].cpu().numpy(), eval_call(ct, NORMAL, DIN, DOUT, N, mask=MASK, exact=exact, mode=1)[k], "eval")
        rgb, cos = ct.eval(din, dout, mask=mask, normal=nrm, cosine=True, exact=exact)
        same_bits(cos.cpu().numpy(), want["cos"], "eval, cosine")
        same_bits(ct.pdf(din, dout, mask=mask, normal=nrm, exact=exact).cpu().numpy(),
                  eval_call(ct, NORMAL, DIN, DOUT, N, mask=MASK, exact=exact, mode=2)["pdf"], "pdf")
        p, cos = ct.pdf(din, dout, mask=mask, normal=nrm, cosine=True, exact=exact)
        same_bits(cos.cpu().numpy(), want["cos"], "pdf, cosine")
        want = eval_call(table, NORMAL, DIN, DOUT, N, mask=MASK, exact=exact, material=MATERIAL)
        rgb, pdf, cos = table.eval_pdf(din, dout, mask=mask, material=ids, normal=nrm, cosine=True, exact=exact)
        got = {"r": rgb[0], "g": rgb[1], "b": rgb[2], "pdf": pdf, "cos": cos}
        same_results({k: v.cpu().numpy() for k, v in got.items()}, want, ("table", exact))
        same_bits(table.pdf(din, dout, mask=mask, material=ids, normal=nrm, exact=exact).cpu().numpy(), want["pdf"],
                  "table pdf")
    # normal=None: today's call
    rgb, pdf = ct.eval_pdf(din, dout, mask=mask, normal=None)
    want = eval_call(ct, None, DIN, DOUT, N, mask=MASK)
    same_bits(rgb[0].cpu().numpy(), want["r"], "local")
    same_bits(pdf.cpu().numpy(), want["pdf"], "local")
    table.close()
    with pytest.raises(ValueError):
        ct.eval_pdf(din, dout, cosine=True)
    with pytest.raises(ValueError, match="to_local"):
        ct.eval_pdf(din, dout, normal=nrm, varying={"roughness": torch.full((N,), 0.2, device="cuda")})
    with pytest.raises(TypeError):
        ct.eval_pdf(din.double(), dout.double(), normal=nrm)
    with pytest.raises(TypeError):
        ct.eval_pdf(din, dout, normal=nrm.double())
    with pytest.raises(ValueError):
        ct.eval_pdf(din, dout, normal=nrm[:, :-1])


@pytest.mark.parametrize("runtime", [False, True])
def test_aggregate_model_is_staged(bbm, runtime):
    tree = bbm.AggregateModel(bbm.Lambertian(albedo=[0.2, 0.5, 0.8]),
                              bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5), runtime=runtime)
    nrm, din, dout, mask = dev(NORMAL), dev(DIN), dev(DOUT), dev(MASK)
    rgb, pdf, cos = tree.eval_pdf(din, dout, mask=mask, normal=nrm, cosine=True)
    li, lo = bbm.to_local(nrm, din, mask), bbm.to_local(nrm, dout, mask)
    rgb0, pdf0 = tree.eval_pdf(li, lo, mask=mask)
    for j in range(3):
        same_bits(rgb[j].cpu().numpy(), rgb0[j].cpu().numpy(), ("tree", runtime, j))
    same_bits(pdf.cpu().numpy(), pdf0.cpu().numpy(), ("tree pdf", runtime))
    same_bits(cos.cpu().numpy(), li[2].cpu().numpy(), ("tree cosine", runtime))
    assert (rgb0[0] != 0).sum() > N // 4
    assert len(tree.eval_pdf(din, dout, mask=mask, normal=nrm)) == 2
    # today's path
    a, b = tree.eval_pdf(din, dout, mask=mask, normal=None), tree.eval_pdf(din, dout, mask=mask)
    same_bits(a[1].cpu().numpy(), b[1].cpu().numpy(), ("tree local", runtime))
