"""The fused sample + eval + weight call (bbm_amd/csrc/sample_eval.hpp: k_sample_eval_v4 / _v1 / _tab / _tab1 behind
bbm_hip_sample_eval, bbm_hip_sample_eval_table and the three Python sample_eval methods).

The contract, lane by lane and bit for bit ("bit for bit" = equal int32 views; NaN lanes compare by where they are NaN,
not by payload): dir / pdf / flag are the sample call's, value is the r, g, b of the eval + pdf call at in = dir, and
weight[c] is numpy float32 (value[c] * dir_z) / pdf where pdf > epsilon and 0 elsewhere.  Every expected value comes
from the staged calls on the same inputs; nothing has a tolerance except the two comparisons that leave the library
(the reference's eval at the parity bar, and a float64 sum taken in another order).

Shared inputs: N = 1217 lanes (4 x 256 + 3 x 64 + 1), `out` from fill_directions over the whole sphere (about half the
lanes below the horizon), xi uniform with lanes 5 and 700 outside [0, 1], a mask with zeros inside one quad and on the
tail.  The library is driven through the C-ABI with every array carved out of one sentinel-filled allocation, 16-byte
aligned (the quad kernel and its scalar tail) or one float further (the one-lane kernel): whatever lies outside the
arrays a call was given must still hold the sentinel afterwards.

A finding of this test's first run: with k_check's div_nr as the weight's quotient, Bagher (golden set 1, lane 699)
returned 1.3805531e-37 where the float32 quotient is 1.3805532e-37; the kernel divides in IEEE arithmetic since.

The weight rule on lanes that are not finite: the issue asks for a weight that is not finite wherever value * dir_z or
pdf is not; the contract's `pdf > epsilon ? ... : 0` gives 0 for a NaN pdf and the IEEE quotient gives 0 for an
infinite one.  The test holds the kernel to the numpy evaluation of the contract's rule (NaN where that is NaN, the same
value elsewhere) and, on top, to the issue's sentence wherever the quotient is formed with a finite pdf.
"""
import ctypes

import numpy as np
import pytest

import bbm_amd
from bbm_amd import check as bcheck
from tests import oracle_util as ou
from tests.test_gpu_loss_models import LAST_FINITE_SET

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
EPS = F(np.finfo(np.float32).eps)
N = 1217                         # 4 * 256 + 3 * 64 + 1
SEED = 0x5EA1
NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
UNSUPPORTED = ["He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"]
SUPPORTED = [n for n in NAMES if n not in UNSUPPORTED]
COMPONENTS = [3, 1, 2]           # All, Diffuse, Specular
SHAPE_ROWS = ["Lambertian", "CookTorrance", "He", "Aggregate<Lambertian,Bagher>"]
SHAPES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027]
REFERENCE_ROWS = ["CookTorrance", "GGX", "Ward", "Aggregate<Lambertian,Bagher>"]
SENTINEL = F(-12345.678)
GUARD = 4                        # floats in front of every array in the arena (keeps the arrays 16-byte aligned)
ROWS = ["dx", "dy", "dz", "pdf", "flag", "r", "g", "b", "wr", "wg", "wb"]
MODE_N = 1 << 20                 # the sampler twins differ on ~1e-5 of CookTorrance's lanes


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


class Common:
    pass


def aligned_rows(t):
    """The rows of a (k, n) tensor as separately allocated 1-D tensors: each one 16-byte aligned whatever n is."""
    return [t[k].clone() for k in range(t.shape[0])]


def make_inputs(bbm, n, seed):
    out = bbm.fill_directions(seed, 1, 0, n, mode=1)             # whole sphere
    g = torch.Generator().manual_seed(seed)
    xi = torch.rand((2, n), generator=g, dtype=torch.float32)
    if n > 700:
        xi[0, 5], xi[1, 700] = 1.5, -0.25
    return aligned_rows(out), aligned_rows(xi.cuda())


@pytest.fixture(scope="module")
def common(bbm):
    c = Common()
    c.out, c.xi = make_inputs(bbm, N, SEED)
    hz = c.out[2].cpu().numpy()
    assert N // 3 < (hz < 0).sum() < 2 * N // 3
    mask = np.ones(N, np.uint8)
    mask[[9, 10, N - 1]] = 0                                     # inside the quad 8..11, and the scalar tail's lane
    c.mask = torch.from_numpy(mask).cuda()
    return c


@pytest.fixture(scope="module")
def merl(bbm, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("merl") / "synthetic.binary")
    ou.synthetic_merl(path)
    return bbm.Merl(path)


def golden_sets(name):
    """The row's first and last golden parameter sets (the last that gives finite values, as the loss and image tests
    choose it); None for a row without golden data."""
    if name not in META:
        return [None]
    g = ou.golden_model(name)
    last = LAST_FINITE_SET.get(name, len(META[name]["sets"]) - 1)
    return [g["params0"].astype(F)] + ([g[f"params{last}"].astype(F)] if last > 0 else [])


@pytest.fixture(scope="module")
def instances(bbm, merl):
    def make(name):
        if name == "Merl":
            return [merl]
        out = []
        for p in golden_sets(name):
            m = bbm.BsdfModel(name)
            if p is not None:
                m.set_parameter_values(p)
            out.append(m)
        return out
    return {name: make(name) for name in NAMES}


def i32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def cut(rows, n):
    return [r[:n] for r in rows]


def fused(m, out, xi, n, comp=3, mask=None, value=True, weight=True, shift=0, exact=None, material=None):
    """bbm_hip_sample_eval (m a BsdfModel) or bbm_hip_sample_eval_table (m a MaterialTable) through the C-ABI on
    the first n lanes.  shift = 1 puts every array one float off its 16-byte boundary.  Returns name -> (n,) numpy
    array of the arrays that were given, after checking that nothing else in the arena was written."""
    lib = bbm_amd._lib.load()
    stride = (GUARD + n + 1 + GUARD + 3) // 4 * 4
    arena = torch.full((len(ROWS) * stride,), float(SENTINEL), dtype=torch.float32, device="cuda")
    given = {k: True for k in ROWS}
    for k in ("r", "g", "b"):
        given[k] = value
    for k in ("wr", "wg", "wb"):
        given[k] = weight
    first = {k: j * stride + GUARD + shift for j, k in enumerate(ROWS)}
    ptr = {k: (arena.data_ptr() + 4 * first[k]) if given[k] else None for k in ROWS}

    def shifted(rows):
        if shift == 0:
            return cut(rows, n)
        keep = [torch.empty(n + 8, dtype=r.dtype, device="cuda") for r in rows]
        res = [b[shift:shift + n] for b in keep]
        for v, r in zip(res, rows):
            v.copy_(r[:n])
        return res
    o, x = shifted(out), shifted(xi)
    mk = None if mask is None else shifted([mask])[0]
    idx = None if material is None else shifted([material])[0]
    for t in o + x:
        assert (t.data_ptr() % 16 == 0) == (shift == 0)
    tail = [mk.data_ptr() if mk is not None else None, n, comp, 0] + [ptr[k] for k in ROWS] + \
           [torch.cuda.current_stream().cuda_stream]
    ins = [t.data_ptr() for t in o + x]
    if material is None:
        rc = lib.bbm_hip_sample_eval(m._call_id(exact), m._pptr(), m._params.size, *ins, *tail)
    else:
        rc = lib.bbm_hip_sample_eval_table(m._live(), m._flags(exact), idx.data_ptr(), *ins, *tail)
    bbm_amd._lib.check(rc)
    host = arena.cpu().numpy()
    touched = np.zeros(host.size, bool)
    res = {}
    for k in ROWS:
        if given[k]:
            touched[first[k]:first[k] + n] = True
            a = host[first[k]:first[k] + n]
            res[k] = a.view(np.uint32) if k == "flag" else a
    rest = host[~touched]
    assert (rest.view(np.int32) == np.asarray(SENTINEL).view(np.int32)).all(), \
        f"{int((rest.view(np.int32) != np.asarray(SENTINEL).view(np.int32)).sum())} floats outside the given arrays written"
    return res


def staged(m, out, xi, n, comp=3, mask=None, **kw):
    """The staged pair on the first n lanes: sample, then eval + pdf (both outputs) at the sampled direction."""
    o, x = cut(out, n), cut(xi, n)
    mk = None if mask is None else mask[:n]
    if "material" in kw:
        kw = dict(kw, material=kw["material"][:n])
    s = m.sample(o, x, comp, mask=mk, **kw)
    v, _ = m.eval_pdf(s.direction, o, comp, mask=mk, **kw)
    d = s.direction.cpu().numpy()
    return {"dx": d[0], "dy": d[1], "dz": d[2], "pdf": s.pdf.cpu().numpy(), "flag": s.flag.cpu().numpy().view(np.uint32),
            "r": v[0].cpu().numpy(), "g": v[1].cpu().numpy(), "b": v[2].cpu().numpy()}


def same_bits(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.dtype == F:
        nan = np.isnan(g)
        assert (nan == np.isnan(w)).all(), (what, "NaN lanes differ", np.nonzero(nan != np.isnan(w))[0][:8])
        g, w = np.where(nan, F(0), g), np.where(nan, F(0), w)
    diff = np.nonzero(g.view(np.int32) != w.view(np.int32))[0]
    assert diff.size == 0, (what, f"{diff.size} lanes differ", diff[:8], g[diff[:4]], w[diff[:4]])


def check_weight(res, what):
    """weight against the numpy float32 rule on the call's own value, dir_z and pdf."""
    v = np.stack([res["r"], res["g"], res["b"]])
    w = np.stack([res["wr"], res["wg"], res["wb"]])
    pdf, dz = res["pdf"][None], res["dz"][None]
    with np.errstate(all="ignore"):
        num = (v * dz).astype(F)
        formed = np.broadcast_to(pdf > EPS, num.shape)
        want = np.where(formed, (num / pdf).astype(F), F(0)).astype(F)
    fin = np.isfinite(num) & np.broadcast_to(np.isfinite(pdf), num.shape)
    for c in range(3):
        same_bits(w[c], want[c], (what, "weight", c))
    # not finite in, not finite out -- wherever the quotient is formed with a finite pdf
    odd = ~fin & formed & np.broadcast_to(np.isfinite(pdf), num.shape)
    assert not np.isfinite(w[odd]).any(), (what, "a finite weight from a value that is not")
    assert (w[~formed] == 0).all() and not np.signbit(w[~formed]).any(), (what, "pdf <= epsilon must give +0")
    return int(fin.sum()), int((~fin).sum())


def compare(res, want, what, value=True):
    for k in ("dx", "dy", "dz", "pdf", "flag") + (("r", "g", "b") if value else ()):
        same_bits(res[k], want[k], (what, k))


def test_rows_are_listed(bbm):
    lib = bbm._lib.load()
    assert len(NAMES) == 49 and len(SUPPORTED) == 43
    assert [n for i, n in enumerate(NAMES) if lib.bbm_hip_model_has_table(i) == 1] == SUPPORTED
    assert set(SHAPE_ROWS) | set(REFERENCE_ROWS) <= set(NAMES)


# ------------------------------------------------------------------------ every row, bit for bit

@pytest.mark.parametrize("name", NAMES)
def test_every_row(bbm, common, instances, name):
    lanes = [0, 0]
    for si, m in enumerate(instances[name]):
        for comp in COMPONENTS:
            what = (name, si, comp)
            res = fused(m, common.out, common.xi, N, comp, common.mask)
            want = staged(m, common.out, common.xi, N, comp, common.mask)
            compare(res, want, what)
            a, b = check_weight(res, what)
            lanes[0] += a
            lanes[1] += b
        # the Python method (its (3, n) outputs are not 16-byte aligned at this n: the one-lane kernel)
        s, v, w = m.sample_eval(common.out, common.xi, mask=common.mask)
        py = {"dx": s.direction[0], "dy": s.direction[1], "dz": s.direction[2], "pdf": s.pdf, "flag": s.flag,
              "r": v[0], "g": v[1], "b": v[2], "wr": w[0], "wg": w[1], "wb": w[2]}
        py = {k: t.cpu().numpy() for k, t in py.items()}
        want = staged(m, common.out, common.xi, N, 3, common.mask)
        compare(py, want, (name, si, "python"))
        check_weight(py, (name, si, "python"))
        assert v.shape == w.shape == (3, N) and s.direction.shape == (3, N)
    print(f"{name}: {lanes[0]} finite weight lanes, {lanes[1]} not finite")


# ------------------------------------------------------------------------ shapes

@pytest.mark.parametrize("name", SHAPE_ROWS)
def test_shapes(bbm, common, instances, name):
    m = instances[name][0]
    for n in SHAPES:
        mask = common.mask if n > 11 else None
        res = fused(m, common.out, common.xi, n, 3, mask)
        want = staged(m, common.out, common.xi, n, 3, mask)
        compare(res, want, (name, n))
        check_weight(res, (name, n))


@pytest.mark.parametrize("name", SHAPE_ROWS)
def test_unaligned_arrays_take_the_one_lane_kernel(bbm, common, instances, name):
    m = instances[name][0]
    n = 257
    res = fused(m, common.out, common.xi, n, 3, common.mask, shift=1)
    want = staged(m, common.out, common.xi, n, 3, common.mask)
    compare(res, want, (name, "shifted"))
    check_weight(res, (name, "shifted"))
    same = fused(m, common.out, common.xi, n, 3, common.mask)
    for k in ROWS:
        same_bits(res[k], same[k], (name, "shifted == aligned", k))


@pytest.mark.parametrize("name", SHAPE_ROWS)
@pytest.mark.parametrize("shift", [0, 1])
def test_each_output_group_alone(bbm, common, instances, name, shift):
    """The group that is stored is unchanged; the other group's place in the arena still holds the sentinel (fused()
    checks every float outside the arrays it gave)."""
    m = instances[name][0]
    n = 257
    both = fused(m, common.out, common.xi, n, 3, common.mask, shift=shift)
    only_v = fused(m, common.out, common.xi, n, 3, common.mask, weight=False, shift=shift)
    only_w = fused(m, common.out, common.xi, n, 3, common.mask, value=False, shift=shift)
    none = fused(m, common.out, common.xi, n, 3, common.mask, value=False, weight=False, shift=shift)
    assert set(only_v) == set(ROWS[:8]) and set(only_w) == set(ROWS[:5] + ROWS[8:]) and set(none) == set(ROWS[:5])
    for res in (only_v, only_w, none):
        for k in res:
            same_bits(res[k], both[k], (name, shift, k))


# ------------------------------------------------------------------------ modes

@pytest.fixture(scope="module")
def mode_inputs(bbm):
    return make_inputs(bbm, MODE_N, SEED + 1)


@pytest.mark.parametrize("name", ["CookTorrance", "GGX"])
def test_exact_and_default_mode(bbm, mode_inputs, name):
    out, xi = mode_inputs
    m = bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.1, eta=1.5) if name == "CookTorrance" else \
        bbm.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.1, eta=1.4)
    got = {}
    for exact in (True, False):
        res = fused(m, out, xi, MODE_N, 3, None, exact=exact)
        want = staged(m, out, xi, MODE_N, 3, None, exact=exact)
        compare(res, want, (name, exact))
        check_weight(res, (name, exact))
        got[exact] = res
    differ = {k: int((i32(got[True][k]) != i32(got[False][k])).sum()) for k in ROWS}
    print(f"{name}: lanes on which exact and default mode differ, per array: {differ}")
    assert sum(differ.values()) > 0, "the two modes agree on every lane: a kernel that ignores the switch would pass"
    # the process-wide switch selects the same kernels as the per-call flag
    prev = bbm.set_exact_subnormals(True)
    try:
        res = fused(m, out, xi, 4099, 3, None)
    finally:
        bbm.set_exact_subnormals(prev)
    for k in ROWS:
        same_bits(res[k], got[True][k][:4099], (name, "process switch", k))


def test_exact_mode_with_an_exact_eval_and_no_sampler_twin(bbm, common, instances):
    """Bagher: model_has_exact, its sampler has no twin."""
    m = instances["Bagher"][0]
    for exact in (True, False):
        res = fused(m, common.out, common.xi, N, 3, common.mask, exact=exact)
        compare(res, staged(m, common.out, common.xi, N, 3, common.mask, exact=exact), ("Bagher", exact))
        check_weight(res, ("Bagher", exact))


def test_runtime_aggregate(bbm, common):
    m = bbm.Aggregate(bbm.Lambertian(albedo=[0.2, 0.5, 0.8]), bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2,
                                                                                 eta=1.5), runtime=True)
    assert isinstance(m, bbm.BsdfModel) and m.runtime and m.name == "Aggregate<Lambertian,CookTorrance>"
    for comp in COMPONENTS:
        res = fused(m, common.out, common.xi, N, comp, common.mask)
        compare(res, staged(m, common.out, common.xi, N, comp, common.mask), ("runtime", comp))
        check_weight(res, ("runtime", comp))


# ------------------------------------------------------------------------ tables

def three_materials(name):
    """Three parameter sets of a row: its golden first and last set and the first scaled by 0.9, clipped to the bounds."""
    sets = golden_sets(name)
    m = bbm_amd.BsdfModel(name)
    base = m.parameter_values().astype(F) if sets[0] is None else sets[0]
    scaled = np.clip(base * F(0.9), m.parameter_lower_bound(), m.parameter_upper_bound()).astype(F)
    return np.stack([base, sets[-1] if sets[-1] is not None else base, scaled])


def material_ids(rng, n, count):
    ids = rng.integers(0, count, n).astype(np.int64)
    ids[[3, 8, n - 1]] = -1                                       # out of range: masked lanes
    ids[[6, 11, n - 2]] = count
    return torch.from_numpy(ids.astype(np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("name", SUPPORTED)
def test_tables(bbm, common, name):
    table = bbm.MaterialTable(name, three_materials(name))
    ids = material_ids(np.random.default_rng(SEED), N, len(table))
    for comp in COMPONENTS:
        res = fused(table, common.out, common.xi, N, comp, common.mask, material=ids)
        want = staged(table, common.out, common.xi, N, comp, common.mask, material=ids)
        compare(res, want, (name, comp))
        check_weight(res, (name, comp))
    res = fused(table, common.out, common.xi, 257, 3, common.mask, material=ids, shift=1)
    compare(res, staged(table, common.out, common.xi, 257, 3, common.mask, material=ids), (name, "shifted"))
    check_weight(res, (name, "shifted"))
    s, v, w = table.sample_eval(common.out, common.xi, mask=common.mask, material=ids, weight=False)
    assert w is None and v.shape == (3, N)
    want = staged(table, common.out, common.xi, N, 3, common.mask, material=ids)
    py = {"dx": s.direction[0], "dy": s.direction[1], "dz": s.direction[2], "pdf": s.pdf, "flag": s.flag,
          "r": v[0], "g": v[1], "b": v[2]}
    compare({k: t.cpu().numpy() for k, t in py.items()}, want, (name, "python"))
    table.close()


@pytest.mark.parametrize("name", UNSUPPORTED)
def test_rows_without_tables(bbm, name):
    lib = bbm._lib.load()
    mid = lib.bbm_hip_model_id(name.encode())
    k = lib.bbm_hip_model_nparams(mid)
    p = (ctypes.c_float * max(3 * k, 1))()
    h = ctypes.c_void_p()
    assert lib.bbm_hip_table_create(mid, p, k, 3, None, ctypes.byref(h)) == bbm._lib.ERR_UNSUPPORTED
    assert h.value is None
    with pytest.raises(bbm._lib.BackboneError) as e:
        bbm.MaterialTable(name, np.zeros((3, k), F))
    assert e.value.code == bbm._lib.ERR_UNSUPPORTED


def test_exact_mode_on_a_table(bbm, common):
    table = bbm.MaterialTable("CookTorrance", three_materials("CookTorrance"))
    ids = material_ids(np.random.default_rng(SEED + 2), N, len(table))
    for exact in (True, False):
        res = fused(table, common.out, common.xi, N, 3, common.mask, material=ids, exact=exact)
        compare(res, staged(table, common.out, common.xi, N, 3, common.mask, material=ids, exact=exact), ("table", exact))


# ------------------------------------------------------------------------ the reference

@pytest.mark.parametrize("name", REFERENCE_ROWS)
def test_value_against_the_reference(bbm, common, instances, name):
    m = instances[name][0]
    res = fused(m, common.out, common.xi, N, 3, None)
    din = np.stack([res["dx"], res["dy"], res["dz"]]).astype(F)
    dout = np.stack([t.cpu().numpy() for t in common.out])
    ref = ou.ref_eval_pdf(name, m.parameter_values(), din, dout)[:3]
    got = np.stack([res["r"], res["g"], res["b"]])
    bad = ou.parity_violations(got, ref)
    print(f"{name}: {len(bad[0])} lanes outside the parity bar of {got.size}; {int((res['flag'] != 0).sum())} samples")
    assert (res["flag"] != 0).sum() > N // 4
    assert len(bad[0]) == 0, (name, bad[1][:8], got[:, bad[1][:4]], ref[:, bad[1][:4]])


# ------------------------------------------------------------------------ checkBsdf's reflectance test

@pytest.mark.parametrize("name", ["CookTorrance", "GGX"])
def test_weight_sums_to_the_reflectance_tests_accumulators(bbm, name):
    """4096 draws of the reflectance test's slot, out = the slot's direction: the float64 sum of the weights over the
    lanes with pdf > epsilon and their count are what bbm_hip_check accumulates with importance sampling.  Only the
    order of 4096 double additions differs: <= 4096 * 2^-53 < 1e-12 relative."""
    m = bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5) if name == "CookTorrance" else \
        bbm.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.3, eta=1.4)
    n, theta, slot = 4096, 4, 2
    outs = bcheck.reflectance_outs(theta)
    acc = bcheck.run(m, bcheck.REFLECTANCE, n, theta, torch.from_numpy(outs).cuda(), bcheck.DEFAULT_SEED,
                     importance=True)[slot]
    xi = bcheck.draws(bcheck.REFLECTANCE, bcheck.DEFAULT_SEED, slot, 0, 0, n)
    out = [torch.full((n,), float(outs[k, slot]), dtype=torch.float32, device="cuda") for k in range(3)]
    res = fused(m, out, aligned_rows(xi), n, 3, None)
    live = res["pdf"] > EPS
    sums = [float(res[k][live].astype(np.float64).sum()) for k in ("wr", "wg", "wb")]
    print(f"{name}: count {int(live.sum())} vs {acc[3]}, sums {sums} vs {list(acc[:3])}")
    assert int(live.sum()) == int(acc[3]) and live.sum() > n // 2
    for c in range(3):
        assert acc[c] > 0 and abs(sums[c] - acc[c]) <= 1e-12 * abs(acc[c]), (name, c, sums[c], acc[c])


# ------------------------------------------------------------------------ streams, trees

def test_side_stream(bbm, common, instances):
    m = instances["CookTorrance"][0]
    s0, v0, w0 = m.sample_eval(common.out, common.xi, mask=common.mask)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    s1, v1, w1 = m.sample_eval(common.out, common.xi, mask=common.mask, stream=side)
    side.synchronize()
    for a, b, k in ((s0.direction, s1.direction, "dir"), (s0.pdf, s1.pdf, "pdf"), (s0.flag, s1.flag, "flag"),
                    (v0, v1, "value"), (w0, w1, "weight")):
        same_bits(a.cpu().numpy().reshape(-1).view(F), b.cpu().numpy().reshape(-1).view(F), k)


@pytest.mark.parametrize("runtime", [False, True])
def test_aggregate_model_is_its_staged_calls(bbm, common, runtime):
    tree = bbm.AggregateModel(bbm.Lambertian(albedo=[0.2, 0.5, 0.8]),
                              bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5),
                              bbm.GGX(albedo=[0.7, 0.6, 0.5], roughness=0.3, eta=1.4), runtime=runtime)
    s, v, w = tree.sample_eval(common.out, common.xi, mask=common.mask)
    want = staged(tree, common.out, common.xi, N, 3, common.mask)
    res = {"dx": s.direction[0], "dy": s.direction[1], "dz": s.direction[2], "pdf": s.pdf, "flag": s.flag,
           "r": v[0], "g": v[1], "b": v[2], "wr": w[0], "wg": w[1], "wb": w[2]}
    res = {k: t.cpu().numpy() for k, t in res.items()}
    res["flag"] = res["flag"].view(np.uint32)
    compare(res, want, ("tree", runtime))
    assert (res["flag"] != 0).sum() > N // 4
    # the rule with torch float32 ops, as the method's docstring says
    rule = torch.where(s.pdf > float(EPS), (v * s.direction[2]) / s.pdf, torch.zeros_like(v)).cpu().numpy()
    for c, k in enumerate(("wr", "wg", "wb")):
        same_bits(res[k], rule[c], ("tree", runtime, k))
    # and the numpy rule wherever the quotient is a normal float or zero
    with np.errstate(all="ignore"):
        q = np.where(res["pdf"][None] > EPS, (v.cpu().numpy() * res["dz"][None]).astype(F) / res["pdf"][None], F(0)).astype(F)
    ok = np.isfinite(q) & ((np.abs(q) >= np.finfo(F).tiny) | (q == 0))
    got = np.stack([res["wr"], res["wg"], res["wb"]])
    assert (got[ok].view(np.int32) == q[ok].view(np.int32)).all()
    s2, v2, w2 = tree.sample_eval(common.out, common.xi, mask=common.mask, value=False)
    assert v2 is None and torch.equal(w2.view(torch.int32), w.view(torch.int32))
