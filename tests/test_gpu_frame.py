"""Per-lane shading frames on the GPU (bbm_amd/csrc/frame.hpp, frame.hip; the FRAME kernels of sample_eval.hpp):
bbm_hip_frame_to_local / _to_global, bbm_hip_sample_eval_world / _table_world and the Python `normal=` surface.

What is held, and to what:
  1. the frame kernel against the image path that is pinned to the reference's renderSphere: bit for bit;
  2. the frame kernel against a float64 numpy restatement of core/shading_frame.h: |error| <= 2^-20 |v| per component
     (about ten float roundings of 2^-24 relative to |v| lie between normal and output; a transposed matrix or a wrong
     sign branch is an O(|v|) error), the same for to_global(to_local(v)) against v;
  3. the identity frame: every normal (0, 0, 1) makes the world call the local call (`==`: -0 equals 0);
  4. fused equals staged -- frame_to_local, the local sample_eval, frame_to_global -- bit for bit on every output
     array, all 49 rows and the 43 table rows;
  5. the Python surface returns the C-ABI results.
"Bit for bit" = equal int32 views; NaN lanes compare by where they are NaN.

Every C-ABI call takes its arrays, inputs included, out of one sentinel-filled allocation, 16-byte aligned (the quad
kernels and their scalar tail) or 4 bytes further (the one-lane kernels); whatever lies outside the call's output
arrays must be unchanged afterwards.

The normals (NORMALS, 1217 lanes): random unit vectors, with these lanes replaced -- (0, 0, 1), (0, 0, -1), (0, 0, 0),
(1, 0, 0), z = -0.0, a normal of length 1e-3 and one of length 1e3 in the first eight lanes (so that every n of the
shape list but 1, 3, 4 and 5 sees all of them, and those see the first ones), and a second (0, 0, 0) on lane 256, the
scalar tail of n = 257.  A (0, 0, 0) lane is not live; in the staged pipeline it is a lane with mask == 0.
"""
import ctypes

import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(np.finfo(np.float32).eps)
N = 1217
SEED = 0xF4A3E
NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
UNSUPPORTED = ["He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"]
SUPPORTED = [n for n in NAMES if n not in UNSUPPORTED]
SHAPES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1217]
SHAPE_ROWS = ["Lambertian", "CookTorrance", "He", "Aggregate<Lambertian,Bagher>"]
SENTINEL = F(-12345.678)
GUARD = 4
OUTS = ["dx", "dy", "dz", "pdf", "flag", "r", "g", "b", "wr", "wg", "wb"]
CAP = 2.0 ** -20


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


# ------------------------------------------------------------------------ the arena

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


def frame_call(to_local, normal, v, n, mask=None, shift=0):
    """bbm_hip_frame_to_local / _to_global on the first n lanes of (3, >= n) numpy arrays -> (3, n)."""
    lib = bbm_amd._lib.load()
    ins = {"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n], "x": v[0][:n], "y": v[1][:n], "z": v[2][:n]}
    if mask is not None:
        ins["mask"] = mask[:n]
    a = Arena(n, shift, ins, ["rx", "ry", "rz"])
    fn = lib.bbm_hip_frame_to_local if to_local else lib.bbm_hip_frame_to_global
    bbm_amd._lib.check(fn(*(a.ptr(k) for k in ("nx", "ny", "nz", "x", "y", "z")),
                          a.ptr("mask") if mask is not None else None, n, a.ptr("rx"), a.ptr("ry"), a.ptr("rz"), stream()))
    r = a.results()
    return np.stack([r["rx"], r["ry"], r["rz"]])


def seval_call(m, normal, out, xi, n, comp=3, mask=None, value=True, weight=True, shift=0, exact=None, material=None):
    """bbm_hip_sample_eval(_table) (normal None) or bbm_hip_sample_eval(_table)_world on the first n lanes."""
    lib = bbm_amd._lib.load()
    ins = {}
    if normal is not None:
        ins.update({"nx": normal[0][:n], "ny": normal[1][:n], "nz": normal[2][:n]})
    ins.update({"ox": out[0][:n], "oy": out[1][:n], "oz": out[2][:n], "xi0": xi[0][:n], "xi1": xi[1][:n]})
    if mask is not None:
        ins["mask"] = mask[:n]
    if material is not None:
        ins["material"] = material[:n]
    given = {k: True for k in OUTS}
    for k in ("r", "g", "b"):
        given[k] = value
    for k in ("wr", "wg", "wb"):
        given[k] = weight
    a = Arena(n, shift, ins, OUTS)
    pre = [a.ptr(k) for k in ("nx", "ny", "nz")] if normal is not None else []
    args = pre + [a.ptr(k) for k in ("ox", "oy", "oz", "xi0", "xi1")] + \
        [a.ptr("mask") if mask is not None else None, n, comp, 0] + [a.ptr(k) if given[k] else None for k in OUTS] + [stream()]
    if material is None:
        fn = lib.bbm_hip_sample_eval if normal is None else lib.bbm_hip_sample_eval_world
        rc = fn(m._call_id(exact), m._pptr(), m._params.size, *args)
    else:
        fn = lib.bbm_hip_sample_eval_table if normal is None else lib.bbm_hip_sample_eval_table_world
        rc = fn(m._live(), m._flags(exact), a.ptr("material"), *args)
    bbm_amd._lib.check(rc)
    return a.results(given)


def live_lanes(normal):
    """|n|^2 > epsilon in the kernel's float32 order."""
    x, y, z = (normal[k].astype(F) for k in range(3))
    with np.errstate(all="ignore"):
        nn = ((F(0) + x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)
    return nn.astype(F) > EPS


def staged(m, normal, out, xi, n, mask=None, shift=0, **kw):
    """frame_to_local, the local call, frame_to_global, every one through the C-ABI with the same mask: the caller's
    with the lanes of a normal that is not live cleared (the contract: such a lane is a masked lane of the pipeline)."""
    mk = (np.ones(n, np.uint8) if mask is None else mask[:n].copy())
    mk[~live_lanes(normal)[:n]] = 0
    lo = frame_call(True, normal, out, n, mk, shift)
    res = seval_call(m, None, lo, xi, n, mask=mk, shift=shift, **kw)
    d = frame_call(False, normal, np.stack([res["dx"], res["dy"], res["dz"]]), n, mk, shift)
    res["dx"], res["dy"], res["dz"] = d[0], d[1], d[2]
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
    for a in v:
        a.flags.writeable = False
    return v


class Common:
    pass


@pytest.fixture(scope="module")
def common(bbm):
    c = Common()
    rng = np.random.default_rng(SEED)
    c.normal = make_normals(rng, N)
    c.out = bbm.fill_directions(SEED, 1, 0, N, mode=1).cpu().numpy()           # world-space, whole sphere
    c.xi = rng.random((2, N), dtype=F)
    c.xi[0, 7], c.xi[1, 700] = 1.5, -0.25
    mask = np.ones(N, np.uint8)
    mask[[9, 10, 254, N - 1]] = 0
    c.mask = mask
    c.vec = (rng.standard_normal((3, N)) * np.exp(rng.uniform(-3, 3, N))).astype(F)     # any length
    ids = rng.integers(0, 5, N).astype(np.int64)
    ids[11] = -1
    c.material = ids.astype(np.uint32)
    for a in (c.out, c.xi, c.mask, c.vec, c.material):
        a.flags.writeable = False
    return c


@pytest.fixture(scope="module")
def merl(bbm, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("merl") / "synthetic.binary")
    ou.synthetic_merl(path)
    return bbm.Merl(path)


def golden_params(name):
    return ou.golden_model(name)["params0"].astype(F) if name in META else None


def instance(bbm, merl, name):
    if name == "Merl":
        return merl
    m = bbm.BsdfModel(name)
    p = golden_params(name)
    if p is not None:
        m.set_parameter_values(p)
    return m


def five_materials(name):
    m = bbm_amd.BsdfModel(name)
    base = golden_params(name)
    base = m.parameter_values().astype(F) if base is None else base
    lo, hi = m.parameter_lower_bound(), m.parameter_upper_bound()
    return np.stack([np.clip(base * F(f), lo, hi).astype(F) for f in (1.0, 0.9, 0.8, 0.95, 0.85)])


def test_rows_are_listed(bbm):
    lib = bbm._lib.load()
    assert len(NAMES) == 49 and len(SUPPORTED) == 43
    assert [n for i, n in enumerate(NAMES) if lib.bbm_hip_model_has_table(i) == 1] == SUPPORTED
    assert set(SHAPE_ROWS) <= set(NAMES)


def test_the_normal_set(common):
    n = common.normal
    ln = np.linalg.norm(n.astype(np.float64), axis=0)
    assert (ln == 0).sum() == 2 and (np.abs(ln - 1e-3) < 1e-9).sum() >= 41 and (np.abs(ln - 1e3) < 1e-3).sum() >= 41
    assert (~live_lanes(n)).sum() == 2 and not live_lanes(n)[2] and not live_lanes(n)[256]
    assert common.mask[2] == 1 and common.mask[256] == 1          # the frame alone switches those lanes off


# ------------------------------------------------------------------------ 1. against the pinned image path

def sphere_normals(w, h):
    """sphere_pixel's normal per pixel (image.hpp; renderSphere.cpp:17-33) in numpy float32.  With radius 8 every
    quotient and |n.xy|^2 are exact; the root is correctly rounded on both sides."""
    radius = F(min(w, h)) / F(2)
    cx, cy = F(w // 2), F(h // 2)
    y, x = np.divmod(np.arange(w * h), w)
    nx = ((cx - x.astype(F)) / radius).astype(F)
    ny = ((cy - y.astype(F)) / radius).astype(F)
    ln = ((F(0) + nx * nx).astype(F) + (ny * ny).astype(F)).astype(F)
    inside = ln < 1
    nz = np.where(inside, np.sqrt(np.where(inside, F(1) - ln, F(0)).astype(F)), F(0)).astype(F)
    return np.stack([np.where(inside, nx, F(0)), np.where(inside, ny, F(0)), nz]).astype(F)


def host_light(light):
    """render_light of the library's host side: -normalize(normalize(light)) in float32."""
    v = np.asarray(light, F)
    for _ in range(2):
        sq = F(F(F(F(0) + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2])
        v = (v * (F(1) / np.sqrt(sq))).astype(F)
    return -v


@pytest.mark.parametrize("shift", [0, 1])
def test_frame_is_the_image_paths(bbm, shift):
    lib = bbm._lib.load()
    w = h = 16
    npix = w * h
    light = (1.0, 2.0, 3.0)
    d = torch.zeros((6, npix), dtype=torch.float32, device="cuda")
    shaded = torch.zeros(npix, dtype=torch.uint8, device="cuda")
    lv = (ctypes.c_float * 3)(*light)
    bbm._lib.check(lib.bbm_hip_render_sphere_dirs(w, h, lv, *(d[k].data_ptr() for k in range(6)), shaded.data_ptr(), stream()))
    d, shaded = d.cpu().numpy(), shaded.cpu().numpy()
    normals = sphere_normals(w, h)
    assert (live_lanes(normals) == (shaded != 0)).all() and 150 < shaded.sum() < 256
    lt = host_light(light)
    got_in = frame_call(True, normals, np.repeat(lt[:, None], npix, 1), npix, shift=shift)
    got_out = frame_call(True, normals, np.repeat(np.array([[0], [0], [1]], F), npix, 1), npix, shift=shift)
    for k in range(3):                                    # every pixel: an unshaded one is 0 on both sides
        same_bits(got_in[k], d[k], ("in", k))
        same_bits(got_out[k], d[3 + k], ("out", k))
    assert (got_in[:, shaded == 0] == 0).all() and np.abs(got_in[:, shaded != 0]).max() > 0.5


# ------------------------------------------------------------------------ 2. against float64 numpy

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


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", SHAPES)
def test_frame_against_float64(common, n, shift):
    nrm, v = common.normal[:, :n], common.vec[:, :n]
    mask = common.mask[:n] if n > 11 else None
    on = live_lanes(nrm) & (np.ones(n, bool) if mask is None else mask != 0)
    X, Y, Z = frame64(nrm)
    v64 = v.astype(np.float64)
    want_l = np.stack([(X * v64).sum(0), (Y * v64).sum(0), (Z * v64).sum(0)])
    want_g = X * v64[0] + Y * v64[1] + Z * v64[2]
    bound = CAP * np.sqrt((v64 * v64).sum(0))
    got_l = frame_call(True, nrm, v, n, mask, shift)
    got_g = frame_call(False, nrm, v, n, mask, shift)
    back = frame_call(False, nrm, got_l, n, mask, shift)
    for got, want, what in ((got_l, want_l, "to_local"), (got_g, want_g, "to_global"), (back, v64, "round trip")):
        err = np.abs(got[:, on].astype(np.float64) - want[:, on])
        print(f"n={n} shift={shift} {what}: max error / |v| = {(err / bound[on] * CAP).max() if on.any() else 0:.3e}")
        assert (err <= bound[on]).all(), (what, n, shift, np.nonzero((err > bound[on]).any(0))[0][:8])
        off = got[:, ~on]
        assert (off.view(np.int32) == 0).all(), (what, "a masked or degenerate lane must write +0")
    # an orthonormal frame keeps lengths
    ln = np.sqrt((got_l[:, on].astype(np.float64) ** 2).sum(0))
    assert np.allclose(ln, np.sqrt((v64[:, on] ** 2).sum(0)), rtol=1e-5, atol=0)


def test_frame_python(bbm, common):
    nrm, v = torch.from_numpy(common.normal.copy()).cuda(), torch.from_numpy(common.vec.copy()).cuda()
    mask = torch.from_numpy(common.mask.copy()).cuda()
    for fn, to_local in ((bbm.to_local, True), (bbm.to_global, False)):
        for mk, mk_np in ((None, None), (mask, common.mask)):
            got = fn(nrm, v, mk)
            assert got.shape == (3, N) and got.dtype == torch.float32
            want = frame_call(to_local, common.normal, common.vec, N, mk_np)
            for k in range(3):
                same_bits(got[k].cpu().numpy(), want[k], (fn.__name__, k))
    with pytest.raises(ValueError):
        bbm.to_local(nrm[:, :-1], v)
    with pytest.raises(TypeError):
        bbm.to_local(nrm, v.double())
    with pytest.raises(ValueError):
        bbm.to_global(nrm, v[:2])


# ------------------------------------------------------------------------ 3. the identity frame

def identity_case(m, common, n, material=None):
    up = np.zeros((3, N), F)
    up[2] = 1
    for exact in (False, True):
        world = seval_call(m, up, common.out, common.xi, n, exact=exact, material=material)
        local = seval_call(m, None, common.out, common.xi, n, exact=exact, material=material)
        for k in OUTS:
            g, w = world[k], local[k]
            nan = np.isnan(g)
            assert (nan == np.isnan(w)).all(), (k, exact)
            bad = np.nonzero(g[~nan] != w[~nan])[0]
            assert bad.size == 0, (k, exact, bad[:8], g[~nan][bad[:4]], w[~nan][bad[:4]])


@pytest.mark.parametrize("name", NAMES)
def test_identity_frame(bbm, common, merl, name):
    identity_case(instance(bbm, merl, name), common, 257)


@pytest.mark.parametrize("name", SUPPORTED)
def test_identity_frame_table(bbm, common, name):
    table = bbm.MaterialTable(name, five_materials(name))
    identity_case(table, common, 257, material=common.material)
    table.close()


# ------------------------------------------------------------------------ 4. fused equals staged

CASES = [dict(value=True, weight=True, mask=True, shift=0), dict(value=False, weight=True, mask=True, shift=1),
         dict(value=True, weight=False, mask=False, shift=0), dict(value=False, weight=False, mask=False, shift=1),
         dict(value=True, weight=True, mask=True, shift=1)]


def fused_is_staged(m, common, n, what, material=None, cases=CASES, modes=(False, True)):
    for exact in modes:
        for c in cases:
            mask = common.mask if c["mask"] else None
            kw = dict(value=c["value"], weight=c["weight"], exact=exact, material=material)
            got = seval_call(m, common.normal, common.out, common.xi, n, mask=mask, shift=c["shift"], **kw)
            want = staged(m, common.normal, common.out, common.xi, n, mask=mask, shift=c["shift"], **kw)
            same_results(got, want, (what, n, exact, tuple(c.items())))
    return got


@pytest.mark.parametrize("name", NAMES)
def test_fused_is_staged(bbm, common, merl, name):
    got = fused_is_staged(instance(bbm, merl, name), common, 257, name)
    # the degenerate lanes (2, and 256 on the scalar tail) and a masked lane: no direction, in any frame
    for lane in (2, 9, 256):
        assert got["dx"][lane] == 0 and got["dy"][lane] == 0 and got["dz"][lane] == 0, lane


@pytest.mark.parametrize("name", SUPPORTED)
def test_fused_is_staged_table(bbm, common, name):
    table = bbm.MaterialTable(name, five_materials(name))
    assert len(table) == 5 and common.material[11] == 0xffffffff
    fused_is_staged(table, common, 257, name, material=common.material)
    table.close()


@pytest.mark.parametrize("name", SHAPE_ROWS)
def test_fused_is_staged_shapes(bbm, common, merl, name):
    m = instance(bbm, merl, name)
    table = bbm.MaterialTable(name, five_materials(name)) if name in SUPPORTED else None
    cases = [dict(value=True, weight=True, mask=True, shift=0), dict(value=True, weight=True, mask=True, shift=1)]
    for n in SHAPES:
        fused_is_staged(m, common, n, name, cases=cases, modes=(False,))
        if table is not None:
            fused_is_staged(table, common, n, name, material=common.material, cases=cases, modes=(False,))
    if table is not None:
        table.close()


def test_degenerate_lane_is_a_masked_lane(bbm, common, merl):
    """The (0, 0, 0) normal with mask 1 gives what the same lane gives with a live normal and mask 0."""
    m = instance(bbm, merl, "CookTorrance")
    n = 257
    a = seval_call(m, common.normal, common.out, common.xi, n, mask=common.mask)
    nrm = common.normal.copy()
    nrm[:, 2] = nrm[:, 256] = (0.0, 0.6, 0.8)
    mask = common.mask.copy()
    mask[[2, 256]] = 0
    b = seval_call(m, nrm, common.out, common.xi, n, mask=mask)
    same_results(a, b, "degenerate == masked")


# ------------------------------------------------------------------------ 5. the Python surface

def py_results(s, v, w):
    res = {"dx": s.direction[0], "dy": s.direction[1], "dz": s.direction[2], "pdf": s.pdf, "flag": s.flag}
    if v is not None:
        res.update({"r": v[0], "g": v[1], "b": v[2]})
    if w is not None:
        res.update({"wr": w[0], "wg": w[1], "wb": w[2]})
    return {k: t.cpu().numpy().view(F) for k, t in res.items()}


def test_python_surface(bbm, common, merl):
    dev = {k: torch.from_numpy(getattr(common, k).copy()).cuda() for k in ("normal", "out", "xi", "mask")}
    ids = torch.from_numpy(common.material.view(np.int32).copy()).cuda()
    ct = instance(bbm, merl, "CookTorrance")
    table = bbm.MaterialTable("CookTorrance", five_materials("CookTorrance"))
    for exact in (None, True):
        got = py_results(*ct.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], normal=dev["normal"], exact=exact))
        same_results(got, seval_call(ct, common.normal, common.out, common.xi, N, mask=common.mask, exact=exact), "model")
        got = py_results(*table.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], material=ids, normal=dev["normal"],
                                            exact=exact))
        same_results(got, seval_call(table, common.normal, common.out, common.xi, N, mask=common.mask, exact=exact,
                                     material=common.material), "table")
    got = py_results(*ct.sample_eval(dev["out"], dev["xi"], normal=dev["normal"], value=False))
    same_results(got, seval_call(ct, common.normal, common.out, common.xi, N, value=False), "weight only")
    # normal=None: today's call
    got = py_results(*ct.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], normal=None))
    same_results(got, seval_call(ct, None, common.out, common.xi, N, mask=common.mask), "local")
    got = py_results(*table.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], material=ids))
    same_results(got, seval_call(table, None, common.out, common.xi, N, mask=common.mask, material=common.material),
                 "local table")
    table.close()
    with pytest.raises(ValueError):
        ct.sample_eval(dev["out"], dev["xi"], normal=dev["normal"][:, :-1])
    with pytest.raises(TypeError):
        ct.sample_eval(dev["out"], dev["xi"], normal=dev["normal"].double())
    with pytest.raises(TypeError):
        ct.sample_eval(dev["out"], dev["xi"], normal=dev["normal"].cpu())


@pytest.mark.parametrize("runtime", [False, True])
def test_aggregate_model_is_staged(bbm, common, runtime):
    tree = bbm.AggregateModel(bbm.Lambertian(albedo=[0.2, 0.5, 0.8]),
                              bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5), runtime=runtime)
    dev = {k: torch.from_numpy(getattr(common, k).copy()).cuda() for k in ("normal", "out", "xi", "mask")}
    s, v, w = tree.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], normal=dev["normal"])
    lo = bbm.to_local(dev["normal"], dev["out"], dev["mask"])
    s0, v0, w0 = tree.sample_eval(lo, dev["xi"], mask=dev["mask"])
    want = py_results(bbm_amd.BsdfSample(bbm.to_global(dev["normal"], s0.direction, dev["mask"]), s0.pdf, s0.flag), v0, w0)
    same_results(py_results(s, v, w), want, ("tree", runtime))
    assert (s.flag != 0).sum() > N // 4
    # today's path
    s1, v1, w1 = tree.sample_eval(dev["out"], dev["xi"], mask=dev["mask"], normal=None)
    s2, v2, w2 = tree.sample_eval(dev["out"], dev["xi"], mask=dev["mask"])
    same_results(py_results(s1, v1, w1), py_results(s2, v2, w2), ("tree local", runtime))
