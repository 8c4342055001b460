"""Material tables (bbm_amd/csrc/table.hpp, the table source of the per-lane kernels in lanes.hpp: k_eval_lane4,
k_eval_lane1, k_sample_lane, k_refl_lane behind bbm_hip_table_* / bbm_hip_*_table and
bbm_amd.MaterialTable).

The contract: lane i's output is what the uniform entry point returns for that pair with material material[i]'s
parameter vector, bit for bit ("bit for bit" = equal int32 views), EPD included; a lane whose index is out of range
is a masked lane.  Every expected value comes from the uniform entry points, called once per material and selected
per lane.  Common inputs: N = 1217 pairs (4 x 256 + 3 x 64 + 1) from fill_directions, `in` on the upper hemisphere
and `out` over the sphere, xi from the library's generator.

  1. every supported row, M = the row's golden parameter sets, indices i % M (mixed within every quad) and random:
     eval_pdf in its three modes, sample and reflectance;
  2. n around the quad, wave and workgroup sizes with one lane moved to another material;
  3. wave-uniform and run-structured indices, M = 1;
  4. out-of-range indices (M, 0x7fffffff, -1) are masked lanes, alone and with a mask;
  5. directions, outputs and indices one element into their buffers (the one-pair kernel);
  6. exact / default mode per call against the process switch, the runtime aggregate baked in at create, component
     and unit;
  7. the published materials of two fits files as one table each;
  8. a 5 000-material table (the implementation has no size threshold: one gather path for every M);
  9. the mixed batch against the reference: zero lanes outside the parity bar;
 10. lifetime: two tables, reuse, a side stream, destroy and create again, create on one stream and use on another;
     and the batch calls' argument errors on a live table;
 11. the table call against the per-lane-rows call over the same parameters: two sources behind shared kernels.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
N = 1217                         # 4 * 256 + 3 * 64 + 1
SEED = 0x7AB1
NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
UNSUPPORTED = {"He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"}
SUPPORTED = [n for n in NAMES if n not in UNSUPPORTED]
SIZE_ROWS = ["CookTorrance", "Aggregate<Lambertian,Bagher>", "EPD"]
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, N]
REFERENCE_ROWS = ["CookTorrance", "GGX", "Ward", "Aggregate<Lambertian,Bagher>"]
FITS_FILES = {"Aggregate<Lambertian,NganCookTorrance>": None, "Aggregate<Lambertian,Bagher>": None}


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


class Common:
    pass


@pytest.fixture(scope="module")
def common(bbm):
    from bbm_amd.plot import plot_draws
    c = Common()
    c.din = bbm.fill_directions(SEED, 0, 0, N, mode=0)          # upper hemisphere
    c.dout = bbm.fill_directions(SEED, 1, 0, N, mode=1)         # whole sphere
    c.xi = plot_draws(SEED, 0, N)
    c.hin, c.hout = c.din.cpu().numpy(), c.dout.cpu().numpy()
    assert (c.hin[2] >= 0).all() and (c.hout[2] < 0).sum() > N // 4
    c.rng = np.random.default_rng(SEED)
    c.mask = torch.from_numpy(c.rng.integers(0, 2, N).astype(np.uint8)).cuda()
    return c


def model_at(name, p, runtime=False):
    m = bbm_amd.BsdfModel(name)
    m.set_parameter_values(p)
    if runtime:
        m.model_id |= bbm_amd._lib.RUNTIME_AGGREGATE
    return m


def sets_of(name):
    """The row's golden parameter sets (params0..), (M, nparams) float32."""
    g = ou.golden_model(name)
    return np.stack([g[f"params{k}"].astype(F) for k in range(len(META[name]["sets"]))])


def ramp(m):
    """m CookTorrance materials: a roughness ramp, albedo and eta moving with it."""
    t = np.linspace(0.0, 1.0, m, dtype=F)
    return np.stack([0.2 + 0.6 * t, 0.8 - 0.5 * t, 0.3 + 0.3 * t, 0.05 + 0.55 * t, 1.3 + 0.4 * t], 1).astype(F)


def i32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def idx_t(assign):
    return torch.from_numpy(np.asarray(assign).astype(np.int64).astype(np.uint32).view(np.int32)).cuda()


def run(m, din, dout, xi, **kw):
    """eval_pdf, reflectance and sample of one call, as a (12, n) int32 array of bits: rgb, pdf, reflectance rgb,
    sample direction, sample pdf, sample flag.  With stream=, the results are read after that stream has finished."""
    rgb, pdf = m.eval_pdf(din, dout, **kw)
    refl = m.reflectance(dout, **kw)
    s = m.sample(dout, xi, **kw)
    if kw.get("stream") is not None:
        kw["stream"].synchronize()
    return np.concatenate([i32(rgb), i32(pdf)[None], i32(refl), i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None]])


def select(per_set, assign):
    """per_set: (M, rows, n); lane i of the result is per_set[assign[i]][:, i]."""
    return per_set[assign, :, np.arange(per_set.shape[2])].T


def per_material(name, sets, din, dout, xi, runtime=False, **kw):
    """The uniform calls, one per material: (M, 12, n) bits."""
    return np.stack([run(model_at(name, p, runtime), din, dout, xi, **kw) for p in sets])


_UNIFORM = {}


def uniform(name, common):
    """per_material of the row's golden sets over the common inputs; computed once."""
    if name not in _UNIFORM:
        _UNIFORM[name] = per_material(name, sets_of(name), common.din, common.dout, common.xi)
    return _UNIFORM[name]


def off1(x):
    """x's rows one element into a buffer of odd pitch: 4-byte aligned, not 16."""
    buf = torch.zeros(x.shape[:-1] + (x.shape[-1] + 1,), dtype=x.dtype, device="cuda")
    buf[..., 1:] = x
    v = buf[..., 1:]
    assert v.data_ptr() % 16 and v.data_ptr() % 4 == 0
    return v


def same(got, want, what):
    diff = np.nonzero((got != want).any(0))[0]
    assert diff.size == 0, (what, f"{diff.size} lanes differ", diff[:8], got[:, diff[:2]], want[:, diff[:2]])


def test_rows_are_listed(bbm):
    assert len(NAMES) == 49 and len(SUPPORTED) == 43 and UNSUPPORTED <= set(NAMES)
    lib = bbm._lib.load()
    assert [n for i, n in enumerate(NAMES) if lib.bbm_hip_model_has_table(i) == 1] == SUPPORTED
    assert set(SIZE_ROWS) | set(REFERENCE_ROWS) | set(FITS_FILES) <= set(SUPPORTED)


# ------------------------------------------------------------------------ 1. every row

@pytest.mark.parametrize("name", SUPPORTED)
def test_every_row(bbm, common, name):
    sets, want = sets_of(name), uniform(name, common)
    M = len(sets)
    assert M >= 2
    t = bbm.MaterialTable(name, sets)
    assert len(t) == M and t.name == name
    # eval alone and pdf alone (eval alone reads the block as the uniform eval does: without host_params)
    one = np.stack([np.concatenate([i32(model_at(name, p).eval(common.din, common.dout)),
                                    i32(model_at(name, p).pdf(common.din, common.dout))[None]]) for p in sets])
    for how, assign in (("mod", np.arange(N) % M), ("random", common.rng.integers(0, M, N))):
        idx = idx_t(assign)
        got = run(t, common.din, common.dout, common.xi, material=idx)
        sel = select(want, assign)
        diff = (got != sel).any(0)
        print(f"{name} {how}: {int(diff.sum())} of {N} lanes differ in some bit")
        same(got, sel, (name, how))
        alone = np.concatenate([i32(t.eval(common.din, common.dout, material=idx)),
                                i32(t.pdf(common.din, common.dout, material=idx))[None]])
        same(alone, select(one, assign), (name, how, "eval / pdf alone"))
    t.close()


# ------------------------------------------------------------------------ 2. batch sizes

@pytest.mark.parametrize("name", SIZE_ROWS)
def test_batch_sizes(bbm, common, name):
    sets, per = sets_of(name), uniform(name, common)
    assert (per[0][:3] != per[1][:3]).any(), "the two materials must differ"
    t = bbm.MaterialTable(name, sets)
    for n in SIZES:
        din, dout, xi = common.din[:, :n].contiguous(), common.dout[:, :n].contiguous(), common.xi[:, :n].contiguous()
        for j in sorted({j for j in (0, n - 1, n // 2) if j < n}):
            assign = np.zeros(n, int)
            assign[j] = 1
            got = run(t, din, dout, xi, material=idx_t(assign))
            want = per[0][:, :n].copy()           # per-pair independent: a prefix of the full batch
            want[:, j] = per[1][:, j]
            same(got, want, (name, n, j))


# ------------------------------------------------------------------------ 3. index structure

@pytest.mark.parametrize("name", ["CookTorrance", "EPD"])
def test_index_structure(bbm, common, name):
    sets, per = sets_of(name), uniform(name, common)
    M = len(sets)
    t = bbm.MaterialTable(name, sets)
    lanes = np.arange(N)
    last_of_wave = np.zeros(N, int)
    last_of_wave[63::64] = 1
    cases = {"one material": np.full(N, M - 1), "runs of 64": (lanes // 64) % M, "runs of 256": (lanes // 256) % M,
             "runs of 100": (lanes // 100) % M, "wave uniform but its last lane": last_of_wave}
    for how, assign in cases.items():
        same(run(t, common.din, common.dout, common.xi, material=idx_t(assign)), select(per, assign), (name, how))
    one = bbm.MaterialTable(name, sets[1:2])
    assert len(one) == 1
    same(run(one, common.din, common.dout, common.xi, material=idx_t(np.zeros(N, int))), per[1], (name, "M = 1"))


# ------------------------------------------------------------------------ 4. out-of-range indices

@pytest.mark.parametrize("name", SIZE_ROWS)
def test_out_of_range_is_a_masked_lane(bbm, common, name):
    sets, per = sets_of(name), uniform(name, common)
    M = len(sets)
    t = bbm.MaterialTable(name, sets)
    assign = common.rng.integers(0, M, N)
    raw = assign.astype(np.int64)
    out = np.zeros(N, bool)
    for k, bad in enumerate((M, 0x7fffffff, -1)):
        where = np.arange(5 + k, N, 7)          # every residue mod 4 and mod 64, first and last quads included
        raw[where] = bad
        out[where] = True
    raw[[0, N - 1]] = -1
    out[[0, N - 1]] = True
    idx = torch.from_numpy(raw.astype(np.int32)).cuda()
    for mask in (None, common.mask):
        hm = np.ones(N, bool) if mask is None else common.mask.cpu().numpy().astype(bool)
        closed = torch.from_numpy((hm & ~out).astype(np.uint8)).cuda()
        # the uniform calls with those lanes masked: what a masked lane returns, and the neighbours unchanged
        want = select(per_material(name, sets, common.din, common.dout, common.xi, mask=closed), assign)
        got = run(t, common.din, common.dout, common.xi, material=idx, mask=mask)
        same(got, want, (name, "masked" if mask is not None else "open"))
        open_ = select(per, assign)
        live = hm & ~out
        assert (got[:, live] == open_[:, live]).all()
        assert not got[:7, ~live].any(), "eval, pdf and reflectance of a masked lane are +0"
    # every index out of range: the whole batch is masked
    got = run(t, common.din, common.dout, common.xi, material=idx_t(np.full(N, -1)))
    want = per_material(name, sets[:1], common.din, common.dout, common.xi, mask=torch.zeros(N, dtype=torch.uint8).cuda())[0]
    same(got, want, (name, "all out of range"))


# ------------------------------------------------------------------------ 5. unaligned arrays

@pytest.mark.parametrize("name", ["CookTorrance", "Aggregate<Lambertian,Bagher>"])
def test_unaligned_arrays(bbm, common, name):
    sets, per = sets_of(name), uniform(name, common)
    M = len(sets)
    t = bbm.MaterialTable(name, sets)
    assign = common.rng.integers(0, M, N)
    want = select(per, assign)
    idx = idx_t(assign)
    uin, uout, uxi, uidx = off1(common.din), off1(common.dout), off1(common.xi), off1(idx)
    rows = lambda v: tuple(v[k] for k in range(v.shape[0]))
    for what, kw in (("directions", dict(din=rows(uin), dout=rows(uout), xi=rows(uxi), material=idx)),
                     ("indices", dict(din=common.din, dout=common.dout, xi=common.xi, material=uidx)),
                     ("all", dict(din=rows(uin), dout=rows(uout), xi=rows(uxi), material=uidx))):
        same(run(t, kw["din"], kw["dout"], kw["xi"], material=kw["material"]), want, (name, what))
    # outputs one element into their buffers
    rgb = off1(torch.zeros((3, N), dtype=torch.float32, device="cuda"))
    pdf = off1(torch.zeros((N,), dtype=torch.float32, device="cuda"))
    t.eval_pdf(common.din, common.dout, material=idx, rgb=rgb, pdf=pdf)
    same(np.concatenate([i32(rgb), i32(pdf)[None]]), want[:4], (name, "outputs"))


# ------------------------------------------------------------------------ 6. modes

def _beckmann_tail_pairs(alpha, count):
    """Pairs mirrored about a half vector tilted by theta_h with tan^2(theta_h) / alpha^2 in [78, 99]: Beckmann's
    exponential is then e^-78 .. e^-99, where the default and the exact mode's quotients round differently."""
    x = np.linspace(78.0, 99.0, count)
    th = np.arctan(np.sqrt(x) * alpha)
    phi = np.linspace(0.1, 6.0, count)
    d = 0.2

    def at(t):
        return np.stack([np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t)]).astype(F)
    return at(th + d), at(th - d)


def test_exact_and_default_mode(bbm, common):
    """CookTorrance at roughness 0.1 with 48 pairs in Beckmann's far tail appended to the batch: the uniform exact
    and default results differ there; the table call follows its flag, whatever the process switch says."""
    name, extra = "CookTorrance", 48
    sets = sets_of(name)[:3].copy()
    sets[:, 3] = 0.1
    sets[1, :3] *= F(0.5)
    tin, tout = _beckmann_tail_pairs(0.1, extra)
    din = torch.cat([common.din, torch.from_numpy(tin).cuda()], 1).contiguous()
    dout = torch.cat([common.dout, torch.from_numpy(tout).cuda()], 1).contiguous()
    from bbm_amd.plot import plot_draws
    n = N + extra
    xi = plot_draws(SEED, 1, n)
    assign = np.arange(n) % len(sets)
    per = {ex: per_material(name, sets, din, dout, xi, exact=ex) for ex in (True, False)}
    differ = (per[True][0][:4, N:] != per[False][0][:4, N:]).any(0)
    print(f"exact and default mode differ on {int(differ.sum())} of the {extra} constructed pairs")
    assert differ.any()
    t = bbm.MaterialTable(name, sets)
    idx = idx_t(assign)
    try:
        for switch in (0, 1):
            bbm.set_exact_subnormals(switch)
            for ex in (True, False):
                same(run(t, din, dout, xi, material=idx, exact=ex), select(per[ex], assign), (switch, ex))
            same(run(t, din, dout, xi, material=idx), select(per[bool(switch)], assign), (switch, None))
    finally:
        bbm.set_exact_subnormals(0)


@pytest.mark.parametrize("name", ["AshikhminShirleyFull", "Aggregate<Lambertian,CookTorrance>", "EPD"])
def test_components_units_and_runtime_aggregate(bbm, common, name):
    sets = sets_of(name)
    assign = common.rng.integers(0, len(sets), N)
    idx = idx_t(assign)
    for runtime in ((False, True) if name.startswith("Aggregate<") else (False,)):
        t = bbm.MaterialTable(name, sets, runtime=runtime)
        assert bool(t.model_id & bbm._lib.RUNTIME_AGGREGATE) == runtime
        for comp, unit in ((bbm.bsdf_flag.Diffuse, bbm.unit_t.Radiance), (bbm.bsdf_flag.Specular, bbm.unit_t.Importance),
                           (bbm.bsdf_flag.All, bbm.unit_t.Importance), (bbm.bsdf_flag.None_, bbm.unit_t.Radiance)):
            want = select(per_material(name, sets, common.din, common.dout, common.xi, runtime=runtime, component=comp,
                                       unit=unit), assign)
            same(run(t, common.din, common.dout, common.xi, material=idx, component=comp, unit=unit), want,
                 (name, runtime, comp, unit))
    if name.startswith("Aggregate<"):
        kids = model_at(name, sets[0]).children()
        models = [bbm.Aggregate(*kids, runtime=True), bbm.Aggregate(*kids, runtime=True)]
        t = bbm.MaterialTable.from_models(models)
        assert len(t) == 2 and t.model_id & bbm._lib.RUNTIME_AGGREGATE


# ------------------------------------------------------------------------ 7. published materials

@pytest.mark.parametrize("key", sorted(FITS_FILES))
def test_published_materials(bbm, common, key):
    with open(os.path.join(ou.ROOT, "tests", "golden", "fits.json")) as f:
        fits = json.load(f)
    fname = sorted(fn for fn, rows in fits.items() if rows and rows[0][2] == key)[0]
    lines = [(s, np.asarray(p, F)) for _, s, k, p in fits[fname] if p is not None and k == key]
    assert 50 <= len(lines) <= 110, (fname, len(lines))
    t = bbm.MaterialTable.from_models([s for s, _ in lines])
    params = np.stack([p for _, p in lines])
    assert len(t) == len(lines) and t.model_id & bbm._lib.RUNTIME_AGGREGATE       # fromString: the runtime aggregate
    assign = common.rng.integers(0, len(lines), N)
    want = select(per_material(key, params, common.din, common.dout, common.xi, runtime=True), assign)
    got = run(t, common.din, common.dout, common.xi, material=idx_t(assign))
    print(f"{fname}: {len(lines)} materials, {int((got != want).any(0).sum())} of {N} lanes differ")
    same(got, want, fname)


# ------------------------------------------------------------------------ 8. a large table

def test_large_table(bbm, common):
    """The gather has one path for every table size (no LDS staging, no size threshold): M = 5 000."""
    name, M = "CookTorrance", 5000
    sets = ramp(M)
    t = bbm.MaterialTable(name, sets)
    assign = common.rng.integers(0, M, N)
    assign[:4] = [0, M - 1, 1, M - 2]
    used, inv = np.unique(assign, return_inverse=True)
    want = select(per_material(name, sets[used], common.din, common.dout, common.xi), inv)
    same(run(t, common.din, common.dout, common.xi, material=idx_t(assign)), want, "M = 5000")


# ------------------------------------------------------------------------ 9. against the reference

@pytest.mark.parametrize("name", REFERENCE_ROWS)
def test_against_the_reference(bbm, common, name):
    sets = sets_of(name)
    t = bbm.MaterialTable(name, sets)
    ref = np.stack([ou.oracle_eval_pdf(name, p, common.hin, common.hout, nthreads=8) for p in sets])
    assign = common.rng.integers(0, len(sets), N)
    rgb, pdf = t.eval_pdf(common.din, common.dout, material=idx_t(assign))
    got = np.concatenate([rgb.cpu().numpy(), pdf.cpu().numpy()[None]])
    want = select(ref, assign)
    bad = ou.parity_violations(got, want)
    print(f"{name}: max rel {np.nanmax(ou.rel_err(got, want)):.3e}, {bad[0].size} lanes outside the bar")
    assert bad[0].size == 0, (name, bad, got[bad], want[bad])


# ------------------------------------------------------------------------ 11. the table source against the rows source

def five_sets(name):
    """M = 5 parameter sets of a row: CookTorrance's ramp, else five points on the segment between the row's first two
    golden sets (the bounds are a box, so every point is a valid set).  EPD: p is material 0's in every set."""
    if name == "CookTorrance":
        return ramp(5)
    s = sets_of(name)
    t = np.linspace(0.0, 1.0, 5, dtype=F)[:, None]
    sets = ((F(1) - t) * s[0] + t * s[1]).astype(F)
    if name == "EPD":
        sets[:, 1] = sets[0, 1]
    assert len(np.unique(sets, axis=0)) == 5
    return sets


@pytest.mark.parametrize("name,exact", [("CookTorrance", False), ("CookTorrance", True),
                                        ("Aggregate<Lambertian,Bagher>", False), ("EPD", False)])
def test_table_and_rows_sources_agree(bbm, common, name, exact):
    """The table and the per-lane-rows calls run the same kernels over two parameter sources (lanes.hpp; only the rows'
    quad eval kernel has a body of its own), so they are held to each other: a table of five sets indexed at random, against the varying call whose rows are those sets
    gathered by the same indices on the host and whose uniform vector is material 0.  eval_pdf, reflectance and sample
    agree bit for bit, under a mask, with every array 16-byte aligned (CookTorrance, EPD: the quad kernels; the
    33-parameter aggregate: the rows' one-pair kernel against the table's quad) and one float into its buffer (the
    one-lane kernels), and an index of -1 is the varying lane with mask = 0.
    EPD's sets share one p.  That is a condition of the comparison, not a tolerance: where p varies per lane the rows
    path takes the device's tgamma for the lanes whose p is not the uniform vector's, the table the host's tgammaf
    per material, and the two round differently."""
    sets = five_sets(name)
    M, P = sets.shape
    assign = common.rng.integers(0, M, N)
    out = np.zeros(N, bool)
    out[3::11] = True                            # every residue mod 4, the first and the last quad, the tail lane
    out[[0, N - 1]] = True
    raw = np.where(out, -1, assign)
    gathered = sets[np.where(out, 0, assign)]    # an index out of range reads the fallback: material 0
    rows = torch.from_numpy(np.ascontiguousarray(gathered.T)).cuda()
    idx = torch.from_numpy(raw.astype(np.int32)).cuda()
    in_range = torch.from_numpy((~out).astype(np.uint8)).cuda()
    t, m = bbm.MaterialTable(name, sets), model_at(name, sets[0])
    tup = lambda v: tuple(v[k] for k in range(v.shape[0]))

    def pitch4(x):
        """x's rows in a buffer whose pitch is a multiple of four floats: every row 16-byte aligned (the rows of a
        (3, N) tensor are not, N being odd)."""
        buf = torch.zeros(x.shape[:-1] + ((x.shape[-1] + 3) & ~3,), dtype=x.dtype, device="cuda")
        buf[..., :x.shape[-1]] = x
        v = buf[..., :x.shape[-1]]
        assert all(r.data_ptr() % 16 == 0 for r in (v if v.dim() == 2 else [v]))
        return v

    def calls(model, din, dout, xi, place, **kw):
        """run(), with eval_pdf writing into buffers placed like the inputs (the quad kernel needs them aligned)."""
        rgb = place(torch.zeros((3, N), dtype=torch.float32, device="cuda"))
        pdf = place(torch.zeros((N,), dtype=torch.float32, device="cuda"))
        model.eval_pdf(din, dout, rgb=rgb, pdf=pdf, **kw)
        refl, s = model.reflectance(dout, **kw), model.sample(dout, xi, **kw)
        return np.concatenate([i32(rgb), i32(pdf)[None], i32(refl), i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None]])

    for what, place in (("aligned", pitch4), ("one float in", off1)):
        din, dout, xi = tup(place(common.din)), tup(place(common.dout)), tup(place(common.xi))
        vrows = place(rows)
        got_t = calls(t, din, dout, xi, place, material=place(idx), mask=common.mask, exact=exact)
        got_v = calls(m, din, dout, xi, place, varying={k: vrows[k] for k in range(P)}, mask=common.mask & in_range,
                      exact=exact)
        open_ = (common.mask.cpu().numpy() != 0) & ~out
        assert got_t[:4, open_].any() and not got_t[:7, ~open_].any(), (name, what)
        same(got_t, got_v, (name, exact, what))
    t.close()


# ------------------------------------------------------------------------ 10. lifetime, arguments

def test_lifetime_and_streams(bbm, common):
    ct, epd = sets_of("CookTorrance"), sets_of("EPD")
    a_ct, a_epd = common.rng.integers(0, len(ct), N), common.rng.integers(0, len(epd), N)
    w_ct, w_epd = select(uniform("CookTorrance", common), a_ct), select(uniform("EPD", common), a_epd)
    t1, t2 = bbm.MaterialTable("CookTorrance", ct), bbm.MaterialTable("EPD", epd)          # two tables alive
    i1, i2 = idx_t(a_ct), idx_t(a_epd)
    for _ in range(2):                                                                      # reuse across calls
        same(run(t1, common.din, common.dout, common.xi, material=i1), w_ct, "two tables: CookTorrance")
        same(run(t2, common.din, common.dout, common.xi, material=i2), w_epd, "two tables: EPD")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = run(t1, common.din, common.dout, common.xi, material=i1, stream=side)
    same(got, w_ct, "side stream")
    # destroy right after the last launch was enqueued, then create again
    rgb, pdf = t1.eval_pdf(common.din, common.dout, material=i1)
    t1.close()
    t1.close()
    with pytest.raises(ValueError):
        t1.eval_pdf(common.din, common.dout, material=i1)
    same(np.concatenate([i32(rgb), i32(pdf)[None]]), w_ct[:4], "destroy after enqueue")
    t1 = bbm.MaterialTable("CookTorrance", ct)
    same(run(t1, common.din, common.dout, common.xi, material=i1), w_ct, "created again")
    # created on stream A, used on stream B after an event wait
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    t3 = bbm.MaterialTable("EPD", epd, stream=sa)
    ev = torch.cuda.Event()
    ev.record(sa)
    sb.wait_event(ev)
    got = run(t3, common.din, common.dout, common.xi, material=i2, stream=sb)
    same(got, w_epd, "stream A -> stream B")
    del t2, t3


def test_argument_errors_on_a_live_table(bbm, common):
    lib, L = bbm._lib.load(), bbm._lib
    t = bbm.MaterialTable("CookTorrance", sets_of("CookTorrance"))
    assert lib.bbm_hip_table_model(t._handle) == t.model_id and lib.bbm_hip_table_size(t._handle) == len(t)
    h, idx = t._handle, idx_t(np.zeros(N, int))
    ip = ctypes.c_void_p(idx.data_ptr())
    d = [ctypes.c_void_p(common.din[k].data_ptr()) for k in range(3)]
    nul7, nul6, nul4 = [None] * 7, [None] * 6, [None] * 4
    calls = {
        "eval_pdf": lambda flags, m, n: lib.bbm_hip_eval_pdf_table(h, flags, m, *nul7, n, 3, 0, None, None, None, None, None),
        "sample": lambda flags, m, n: lib.bbm_hip_sample_table(h, flags, m, *nul6, n, 3, 0, None, None, None, None, None, None),
        "reflectance": lambda flags, m, n: lib.bbm_hip_reflectance_table(h, flags, m, *nul4, n, 3, 0, None, None, None, None),
    }
    for name, f in calls.items():
        assert f(0, None, 0) == 0 and f(L.CALL_EXACT, ip, 0) == 0, name                  # n == 0 is a no-op
        assert f(0, None, 16) == L.ERR_INVALID_ARG and b"material" in lib.bbm_hip_last_error(), name
        assert f(0, ip, 16) == L.ERR_INVALID_ARG and b"direction" in lib.bbm_hip_last_error(), name
        for flags in (L.CALL_EXACT | L.CALL_DEFAULT, L.RUNTIME_AGGREGATE, 1):
            assert f(flags, ip, 16) == L.ERR_INVALID_ARG and b"call_flags" in lib.bbm_hip_last_error(), (name, flags)
    # every output NULL
    assert lib.bbm_hip_eval_pdf_table(h, 0, ip, *d, *d, None, 16, 3, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    # Python: index dtype / device -> TypeError, shape / length / stride -> ValueError, float64 -> TypeError
    din, dout, xi = common.din, common.dout, common.xi
    calls = [lambda i, **kw: t.eval_pdf(din, dout, material=i, **kw), lambda i, **kw: t.eval(din, dout, material=i, **kw),
             lambda i, **kw: t.pdf(din, dout, material=i, **kw), lambda i, **kw: t.sample(dout, xi, material=i, **kw),
             lambda i, **kw: t.reflectance(dout, material=i, **kw)]
    for f in calls:
        with pytest.raises(TypeError):
            f(idx.long())
        with pytest.raises(TypeError):
            f(idx.cpu())
        with pytest.raises(TypeError):
            f(idx.cpu().numpy())
        with pytest.raises(ValueError):
            f(idx[:-1])
        with pytest.raises(ValueError):
            f(idx.reshape(1, N))
        with pytest.raises(ValueError):
            f(torch.zeros((N, 2), dtype=torch.int32, device="cuda")[:, 0])
    with pytest.raises(TypeError):
        t.eval_pdf(din.double(), dout.double(), material=idx)
    with pytest.raises(TypeError):
        t.sample(dout.double(), xi.double(), material=idx)
    with pytest.raises(TypeError):
        t.reflectance(dout.double(), material=idx)
