"""Per-lane model parameters (bbm_amd/csrc/varying.hpp, the rows source of lanes.hpp's k_eval_pdf_var, k_eval_lane1,
k_sample_lane and k_refl_lane, behind bbm_hip_*_varying and the `varying=` keyword of BsdfModel).

The contract: lane i's output is what the uniform entry point returns for that pair at lane i's parameter vector, bit
for bit ("bit for bit" = equal int32 views, so NaN for NaN).  Common inputs: N = 1217 pairs (4 x 256 + 3 x 64 + 1)
from fill_directions, `in` on the upper hemisphere and `out` over the sphere, xi from the library's generator; K = 3
parameter sets per row (the golden file's first set, its last -- for Ribardiere and Bagher the set LAST_FINITE_SET
names -- and the first scaled by 0.9 and clipped to the bounds).

  1. every supported row, all parameters varying, sets assigned i % 3 and at random: eval_pdf, reflectance and sample
     equal the three uniform calls selected per lane; EPD with p varying is held to the per-lane parity bar against the
     uniform result (its normalization's tgamma), and bit for bit with p uniform;
  2. eval-only and pdf-only equal the fused call's halves;
  3. some parameters varying (an attribute name, a (3, n) attribute, integer indices) equal the all-rows form with the
     other rows broadcast, and the uniform calls; component flags and a runtime fused aggregate's id pass through;
  4. n around the quad, wave and workgroup sizes: a constant row equals the uniform call; one lane at another set
     changes that lane only, to the other set's uniform value; rows one float into a buffer (4-byte aligned) equal
     the aligned copy's result.  No new kernel runs a capped grid, so there is no second grid-stride trip to force;
  5. masked lanes are zero, the others unchanged;
  6. exact mode: varying equals uniform in both modes, on a batch where the two modes differ;
  7. the mixed batch against the reference evaluated per set: zero lanes outside the parity bar;
  8. argument errors raise before a launch; a side stream gives the default stream's result.
"""
import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
N = 1217                         # 4 * 256 + 3 * 64 + 1
K = 3
SEED = 0x7A21
NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
UNSUPPORTED = {"He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"}
SUPPORTED = [n for n in NAMES if n not in UNSUPPORTED]
# tests/test_gpu_loss_models.py: the last golden set of these rows that gives finite values
LAST_FINITE_SET = {"Ribardiere": 0, "Bagher": 1}
# tests/test_gpu_image_models.py: rows with an exact instantiation (the leaf, alone or in Aggregate<Lambertian, leaf>)
EXACT_EVAL_LEAVES = {"CookTorrance", "LowCookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "NganCookTorrance",
                     "Ribardiere", "RibardiereAnisotropic", "LowMicrofacet", "LowMicrofacetFit", "LowSmooth", "Bagher"}
EXACT_SAMPLE_LEAVES = {"CookTorrance", "LowCookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "NganCookTorrance",
                       "GGX", "GGXHeitz"}
MODE_ROWS = ["Lambertian", "CookTorrance", "AshikhminShirleyFull", "Aggregate<Lambertian,Bagher>"]
TAIL_ROWS = ["Lambertian", "CookTorrance", "Aggregate<Lambertian,Bagher>"]
TAIL_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, N]
REFERENCE_ROWS = ["CookTorrance", "GGX", "Ward", "Aggregate<Lambertian,Bagher>"]


def _leaf(name):
    return name[len("Aggregate<Lambertian,"):-1] if name.startswith("Aggregate<Lambertian,") else name


EXACT_ROWS = [n for n in SUPPORTED if _leaf(n) in EXACT_EVAL_LEAVES | EXACT_SAMPLE_LEAVES]


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
    rng = np.random.default_rng(SEED)
    c.assign = {"mod3": np.arange(N) % K, "random": rng.integers(0, K, N)}
    c.mask = torch.from_numpy(rng.integers(0, 2, N).astype(np.uint8)).cuda()
    return c


def model_at(name, p, like=None):
    m = bbm_amd.BsdfModel(name)
    m.set_parameter_values(p)
    if like is not None:
        m.model_id = like.model_id
    return m


_SETS = {}


def sets_of(name):
    """The row's K parameter sets, (K, nparams) float32."""
    if name not in _SETS:
        m = bbm_amd.BsdfModel(name)
        if name in META:
            g = ou.golden_model(name)
            last = LAST_FINITE_SET.get(name, len(META[name]["sets"]) - 1)
            first, second = g["params0"].astype(F), g[f"params{last}"].astype(F)
        else:
            first = second = m.parameter_values()
        third = np.clip(first * F(0.9), m.parameter_lower_bound(), m.parameter_upper_bound()).astype(F)
        _SETS[name] = np.stack([first, second, third])
    return _SETS[name]


def i32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def run(m, din, dout, xi, **kw):
    """eval_pdf, reflectance and sample of one call, as a (12, n) int32 array of bits: rgb, pdf, reflectance rgb,
    sample direction, sample pdf, sample flag."""
    rgb, pdf = m.eval_pdf(din, dout, **kw)
    refl = m.reflectance(dout, **kw)
    s = m.sample(dout, xi, **kw)
    return np.concatenate([i32(rgb), i32(pdf)[None], i32(refl), i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None]])


def rows_of(params, assign):
    """(nparams, n) float32 CUDA rows: lane i carries params[assign[i]]."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(params, F)[assign].T)).cuda()


def all_rows(rows):
    return {k: rows[k] for k in range(rows.shape[0])}


def select(per_set, assign):
    """per_set: (K, rows, n); lane i of the result is per_set[assign[i]][:, i]."""
    return per_set[assign, :, np.arange(per_set.shape[2])].T


_UNIFORM = {}


def uniform(name, common, exact=None):
    """The K uniform calls of the row over the common inputs, (K, 12, N) bits; computed once."""
    key = (name, exact)
    if key not in _UNIFORM:
        _UNIFORM[key] = np.stack([run(model_at(name, p), common.din, common.dout, common.xi, exact=exact)
                                  for p in sets_of(name)])
    return _UNIFORM[key]


def test_rows_are_listed(bbm):
    assert len(NAMES) == 49 and len(SUPPORTED) == 43 and UNSUPPORTED <= set(NAMES)
    assert set(MODE_ROWS) | set(TAIL_ROWS) | set(REFERENCE_ROWS) <= set(SUPPORTED)
    lib = bbm._lib.load()
    assert [n for i, n in enumerate(NAMES) if lib.bbm_hip_model_has_varying(i) == 1] == SUPPORTED
    with pytest.raises(bbm._lib.BackboneError) as e:
        bbm.BsdfModel("He").eval_pdf(bbm.fill_directions(1, 0, 0, 8), bbm.fill_directions(1, 1, 0, 8), varying={})
    assert e.value.code == bbm._lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------ 1. every row, every parameter varying

@pytest.mark.parametrize("name", SUPPORTED)
def test_all_parameters_varying(bbm, common, name):
    sets, want = sets_of(name), uniform(name, common)
    m = model_at(name, sets[0])
    for how, assign in common.assign.items():
        got = run(m, common.din, common.dout, common.xi, varying=all_rows(rows_of(sets, assign)))
        sel = select(want, assign)
        if name == "EPD":
            # p varies: a lane whose p is not the call's uniform p takes the correctly rounded tgamma(1 / p) where the
            # uniform call takes glibc's tgammaf from the host, so its normalization may be an ulp off (EpdNdf)
            gf, wf = got[:11].view(F), sel[:11].view(F)
            bad = ou.parity_violations(gf, wf)
            print(f"EPD {how}: {int((got != sel).any(0).sum())} of {N} lanes differ in some bit, "
                  f"max rel {np.nanmax(ou.rel_err(gf, wf)):.3e}")
            assert bad[0].size == 0, (name, how, bad)
            assert (got[11] == sel[11]).all()
            lanes = assign == 0          # the uniform p is set 0's: those lanes take the host value
            assert (got[:, lanes] == sel[:, lanes]).all(), (name, how)
        else:
            diff = np.nonzero((got != sel).any(0))[0]
            assert diff.size == 0, (name, how, diff[:8], got[:, diff[:2]], sel[:, diff[:2]])


def test_epd_with_uniform_p(bbm, common):
    """EPD with p uniform and beta, eta varying: bit for bit."""
    sets = sets_of("EPD").copy()
    sets[:, 1] = sets[0, 1]
    want = np.stack([run(model_at("EPD", p), common.din, common.dout, common.xi) for p in sets])
    m = model_at("EPD", sets[0])
    for how, assign in common.assign.items():
        rows = rows_of(sets, assign)
        got = run(m, common.din, common.dout, common.xi, varying={0: rows[0], 2: rows[2], 3: rows[3]})
        assert (got == select(want, assign)).all(), how
        got = run(m, common.din, common.dout, common.xi, varying={"beta": rows[0], "eta": rows[2:4]})
        assert (got == select(want, assign)).all(), how


# ------------------------------------------------------------------------ 2. modes

@pytest.mark.parametrize("name", MODE_ROWS)
def test_eval_only_and_pdf_only(bbm, common, name):
    sets = sets_of(name)
    m = model_at(name, sets[0])
    v = all_rows(rows_of(sets, common.assign["mod3"]))
    rgb, pdf = m.eval_pdf(common.din, common.dout, varying=v)
    assert (i32(m.eval(common.din, common.dout, varying=v)) == i32(rgb)).all()
    assert (i32(m.pdf(common.din, common.dout, varying=v)) == i32(pdf)).all()
    want = select(uniform(name, common), common.assign["mod3"])
    assert (i32(rgb) == want[:3]).all() and (i32(pdf) == want[3]).all()


# ------------------------------------------------------------------------ 3. some parameters varying

def test_partial_cooktorrance(bbm, common):
    name = "CookTorrance"
    sets, assign = sets_of(name), common.assign["random"]
    m = model_at(name, sets[0])
    rows = rows_of(sets, assign)
    base = rows_of(sets[:1], np.zeros(N, int))
    for key, slots in (("roughness", [3]), ("albedo", [0, 1, 2])):
        mixed = sets[[0, 0, 0]].copy()
        mixed[:, slots] = sets[:, slots]
        want = select(np.stack([run(model_at(name, p), common.din, common.dout, common.xi) for p in mixed]), assign)
        part = rows[slots[0]] if len(slots) == 1 else rows[slots[0]:slots[-1] + 1]
        got = run(m, common.din, common.dout, common.xi, varying={key: part})
        full = base.clone()
        full[slots] = rows[slots]
        broadcast = run(m, common.din, common.dout, common.xi, varying=all_rows(full))
        assert (got == want).all() and (got == broadcast).all(), key
        assert (got != uniform(name, common)[0]).any(), key


def test_partial_aggregate_indices(bbm, common):
    name = "Aggregate<Lambertian,Bagher>"
    sets, assign = sets_of(name), common.assign["random"]
    assert bbm.BsdfModel(name).parameter_values().size == 33
    m = model_at(name, sets[0])
    rows = rows_of(sets, assign)
    slots = [1, 21, 32]          # Lambertian's green albedo, Bagher's first alpha, its last Fresnel offset
    mixed = sets[[0, 0, 0]].copy()
    mixed[:, slots] = sets[:, slots]
    want = select(np.stack([run(model_at(name, p), common.din, common.dout, common.xi) for p in mixed]), assign)
    got = run(m, common.din, common.dout, common.xi, varying={k: rows[k] for k in slots})
    full = rows_of(sets[:1], np.zeros(N, int))
    full[slots] = rows[slots]
    broadcast = run(m, common.din, common.dout, common.xi, varying=all_rows(full))
    assert (got == want).all() and (got == broadcast).all()
    assert (got != uniform(name, common)[0]).any()


@pytest.mark.parametrize("name", ["AshikhminShirleyFull", "Aggregate<Lambertian,CookTorrance>"])
def test_components_and_runtime_aggregate(bbm, common, name):
    sets, assign = sets_of(name), common.assign["mod3"]
    models = [model_at(name, sets[0])]
    if name.startswith("Aggregate<"):
        kids = models[0].children()
        models.append(bbm.Aggregate(*kids, runtime=True))
        assert models[1].runtime and models[1].name == name
    v = all_rows(rows_of(sets, assign))
    for m in models:
        for comp in (bbm.bsdf_flag.Diffuse, bbm.bsdf_flag.Specular, bbm.bsdf_flag.All):
            want = select(np.stack([run(model_at(name, p, like=m), common.din, common.dout, common.xi, component=comp)
                                    for p in sets]), assign)
            got = run(m, common.din, common.dout, common.xi, component=comp, varying=v)
            assert (got == want).all(), (name, m.runtime, comp)


# ------------------------------------------------------------------------ 4. indexing and tails

@pytest.mark.parametrize("name", TAIL_ROWS)
def test_indexing_and_tails(bbm, common, name):
    sets = sets_of(name)
    m = model_at(name, sets[0])
    per_set = uniform(name, common)
    assert (per_set[0][:3] != per_set[1][:3]).any(), "the two sets must differ"
    for n in TAIL_N:
        din, dout, xi = common.din[:, :n].contiguous(), common.dout[:, :n].contiguous(), common.xi[:, :n].contiguous()
        base = run(m, din, dout, xi)
        assert (base == per_set[0][:, :n]).all(), n           # per-pair independent: a prefix of the full batch
        other = per_set[1][:, :n]
        const = rows_of(sets[:1], np.zeros(n, int))
        assert (run(m, din, dout, xi, varying=all_rows(const)) == base).all(), n
        for j in sorted({j for j in (0, n - 1, 63, 64, 255, 256) if j < n}):
            assign = np.zeros(n, int)
            assign[j] = 1
            rows = rows_of(sets, assign)
            got = run(m, din, dout, xi, varying=all_rows(rows))
            want = base.copy()
            want[:, j] = other[:, j]
            assert (got == want).all(), (name, n, j, np.nonzero((got != want).any(0))[0][:8])
            if j in (0, n - 1):
                # the same rows one float into a buffer: 4-byte aligned, not 16 (rows of odd pitch n + 1)
                buf = torch.zeros((rows.shape[0], n + 1), dtype=torch.float32, device="cuda")
                buf[:, 1:] = rows
                views = {k: buf[k, 1:] for k in range(rows.shape[0])}
                assert any(v.data_ptr() % 16 for v in views.values()) and all(v.data_ptr() % 4 == 0 for v in views.values())
                assert (run(m, din, dout, xi, varying=views) == want).all(), (name, n, j, "unaligned")


# ------------------------------------------------------------------------ 5. mask

@pytest.mark.parametrize("name", TAIL_ROWS)
def test_mask(bbm, common, name):
    sets, assign = sets_of(name), common.assign["random"]
    m = model_at(name, sets[0])
    hm = common.mask.cpu().numpy().astype(bool)
    assert hm.any() and (~hm).any()
    want = select(np.stack([run(model_at(name, p), common.din, common.dout, common.xi, mask=common.mask) for p in sets]),
                  assign)
    got = run(m, common.din, common.dout, common.xi, mask=common.mask, varying=all_rows(rows_of(sets, assign)))
    assert (got == want).all()
    open_ = select(uniform(name, common), assign)
    assert not got[:7, ~hm].any(), "eval, pdf and reflectance of a masked lane are +0"
    assert (got[:, hm] == open_[:, hm]).all()


# ------------------------------------------------------------------------ 6. exact mode

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


@pytest.mark.parametrize("name", EXACT_ROWS)
def test_exact_mode(bbm, common, name):
    sets = sets_of(name)
    m = model_at(name, sets[0])
    for how, assign in common.assign.items():
        v = all_rows(rows_of(sets, assign))
        for exact in (True, False):
            got = run(m, common.din, common.dout, common.xi, exact=exact, varying=v)
            assert (got == select(uniform(name, common, exact), assign)).all(), (name, how, exact)


def test_exact_mode_is_not_ignored(bbm, common):
    """CookTorrance at roughness 0.1 with 48 pairs in Beckmann's far tail appended to the batch: the uniform exact and
    default results differ there, and the varying call follows the mode it is given."""
    name, extra = "CookTorrance", 48
    sets = sets_of(name).copy()
    sets[:, 3] = [0.1, 0.1, 0.1]
    sets[1, :3] *= F(0.5)
    tin, tout = _beckmann_tail_pairs(0.1, extra)
    din = torch.cat([common.din, torch.from_numpy(tin).cuda()], 1).contiguous()
    dout = torch.cat([common.dout, torch.from_numpy(tout).cuda()], 1).contiguous()
    n = N + extra
    assign = np.arange(n) % K
    def eval_pdf_bits(mm, **kw):
        rgb, pdf = mm.eval_pdf(din, dout, **kw)
        return np.concatenate([i32(rgb), i32(pdf)[None]])
    per = {ex: np.stack([eval_pdf_bits(model_at(name, p), exact=ex) for p in sets]) for ex in (True, False)}
    tail = slice(N, n)
    differ = (per[True][0][:, tail] != per[False][0][:, tail]).any(0)
    print(f"exact and default mode differ on {int(differ.sum())} of the {extra} constructed pairs")
    assert differ.any()
    m = model_at(name, sets[0])
    v = all_rows(rows_of(sets, assign))
    for ex in (True, False):
        assert (eval_pdf_bits(m, exact=ex, varying=v) == select(per[ex], assign)).all(), ex


# ------------------------------------------------------------------------ 7. against the reference

@pytest.mark.parametrize("name", REFERENCE_ROWS)
def test_against_the_reference(bbm, common, name):
    sets = sets_of(name)
    m = model_at(name, sets[0])
    ref = np.stack([ou.oracle_eval_pdf(name, p, common.hin, common.hout, nthreads=8) for p in sets])
    for how, assign in common.assign.items():
        rgb, pdf = m.eval_pdf(common.din, common.dout, varying=all_rows(rows_of(sets, assign)))
        got = np.concatenate([rgb.cpu().numpy(), pdf.cpu().numpy()[None]])
        want = select(ref, assign)
        bad = ou.parity_violations(got, want)
        print(f"{name} {how}: max rel {np.nanmax(ou.rel_err(got, want)):.3e}, {bad[0].size} lanes outside the bar")
        assert bad[0].size == 0, (name, how, bad, got[bad], want[bad])


# ------------------------------------------------------------------------ 8. arguments, streams

def test_python_argument_errors(bbm, common):
    m = bbm.CookTorrance()
    din, dout, xi = common.din, common.dout, common.xi
    row = torch.full((N,), 0.2, dtype=torch.float32, device="cuda")
    calls = [lambda v: m.eval_pdf(din, dout, varying=v), lambda v: m.eval(din, dout, varying=v),
             lambda v: m.pdf(din, dout, varying=v), lambda v: m.sample(dout, xi, varying=v),
             lambda v: m.reflectance(dout, varying=v)]
    for f in calls:
        with pytest.raises(TypeError):
            f({"sharpness": row})                                  # unknown attribute
        with pytest.raises(ValueError):
            f({5: row})                                            # index out of range
        with pytest.raises(ValueError):
            f({-1: row})
        with pytest.raises(ValueError):
            f({"albedo": row})                                     # (3, n) expected
        with pytest.raises(ValueError):
            f({"roughness": row[:-1]})                             # wrong length
        with pytest.raises(ValueError):
            f({"roughness": torch.zeros((N, 2), dtype=torch.float32, device="cuda")[:, 0]})    # strided row
        with pytest.raises(ValueError):
            f({"roughness": row, 3: row})                          # the same slot twice
        with pytest.raises(TypeError):
            f({"roughness": row.double()})                         # dtype
        with pytest.raises(TypeError):
            f({"roughness": row.cpu()})                            # device
    with pytest.raises(TypeError):
        bbm.BsdfModel("Aggregate<Lambertian,CookTorrance>").eval_pdf(din, dout, varying={"roughness": row})
    d64 = (din.double(), dout.double(), xi.double())
    with pytest.raises(TypeError):
        m.eval_pdf(d64[0], d64[1], varying={"roughness": row})     # doubleRGB is out of scope
    with pytest.raises(TypeError):
        m.sample(d64[1], d64[2], varying={"roughness": row})
    with pytest.raises(TypeError):
        m.reflectance(d64[1], varying={"roughness": row})
    for agg in (bbm.AggregateModel(bbm.Lambertian(), bbm.CookTorrance()),
                bbm.AggregateModel(bbm.Lambertian(), bbm.CookTorrance(), runtime=True)):
        with pytest.raises(NotImplementedError):
            agg.eval_pdf(din, dout, varying={0: row})
        with pytest.raises(NotImplementedError):
            agg.eval(din, dout, varying={0: row})
        with pytest.raises(NotImplementedError):
            agg.sample(dout, xi, varying={0: row})
        with pytest.raises(NotImplementedError):
            agg.reflectance(dout, varying={0: row})
    # an empty mapping is the uniform call
    assert (run(m, din, dout, xi, varying={}) == run(m, din, dout, xi)).all()


def test_side_stream(bbm, common):
    name = "CookTorrance"
    sets, assign = sets_of(name), common.assign["random"]
    m = model_at(name, sets[0])
    rows = rows_of(sets, assign)
    want = run(m, common.din, common.dout, common.xi, varying=all_rows(rows))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    rgb, pdf = m.eval_pdf(common.din, common.dout, varying=all_rows(rows), stream=side)
    refl = m.reflectance(common.dout, varying=all_rows(rows), stream=side)
    s = m.sample(common.dout, common.xi, varying=all_rows(rows), stream=side)
    side.synchronize()
    got = np.concatenate([i32(rgb), i32(pdf)[None], i32(refl), i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None]])
    assert (got == want).all()
