"""Every registry row through the fused fitting-loss kernels (bbm_amd/csrc/kernels.hpp launch_loss<M>: k_loss_models,
the pair-major k_loss_pairs, the probe-batch k_loss, k_loss_final), at small n and with exact identities where they
exist -- a sum over 10^5 samples held to 1e-5 cannot see one dropped or doubled sample.

Common inputs: N = 1217 pairs (four full workgroups, three waves and one lane) from fill_directions, `in` on the upper
hemisphere and `out` over the whole sphere; the "far" reference table GGX(roughness = 0.2) (CookTorrance for the GGX
rows); three probes per row (its parameters and two copies scaled by 0.9 and 1.1, clipped to the bounds; Merl its one
vector three times).  Every staged per-sample loss of every row is finite on these pairs (common()).

  1. every row, six loss kinds: fused probe sums == the staged pipeline (m.eval on the GPU, the per-sample losses in
     numpy float32, summed in float64) at REL = 1e-5; and, for the rows the oracle's bbmref_loss knows, == the
     reference's own per-sample losses on the same pairs at REL;
  2. every row, six kinds: fused probe sums == the one-leaf tree path (bbm_hip_loss_tree: the eval kernels plus
     k_loss_terms) to rtol 1e-12 (the summation order), REL for the rows of NOT_BITWISE;
  3. every row: with the row's own eval as the reference table and its own parameters as the probe, all six sums are
     exactly 0.0 -- the loss kernels' eval is the eval kernels', bit for bit -- and the same at each scaled copy of
     the parameters against its own eval; except the rows of NOT_BITWISE, which are then not all zero (the list is
     asserted both ways);
  4. per-sample indexing: a reference table that differs from the row's eval at one sample gives, bit for bit, the sum
     of a launch over that pair alone -- n from 1 to 1217 around the wave and workgroup sizes, and n = 600 001 (grid
     capped at kLossMaxBlocks, whole device-fulls, unequal shares);
  5. the probe-batch kernel k_loss (1537 probes) == the same probes in two pair-major launches, rtol 1e-12, and the
     staged value at REL;
  6. the in-kernel linearizer on a shard (begin != 0, n no multiple of 256) == bbm_hip_loss_pairs over the
     materialised pairs, bit for bit; n = 0 returns BBM_HIP_OK and sums of exactly 0.0;
  7. component Diffuse / Specular / All through the loss kernels == the staged pipeline at REL.
"""
import ctypes

import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
META_FIT, _FIT = ou.golden_fit()
F = np.float32
REL = 1e-5                       # the project's bar (tests/test_gpu_fit.py)
ORDER = 1e-12                    # double sums of 1217 non-negative terms in another order: <= ~1217 * 2^-53
N = 1217                         # 4 * 256 + 3 * 64 + 1
SPARE = 12                       # 1 % of N: candidate pairs beyond N that may replace non-finite ones
SEED = 0x1055
KINDS = range(6)
GGX_ROWS = {"GGX", "GGXHeitz", "Aggregate<Lambertian,GGX>"}
AGGREGATES = [n for n in NAMES if n.startswith("Aggregate<Lambertian,")]

# Rows whose loss kernels do not evaluate the eval kernels' floats (part 3).
NOT_BITWISE = {
    # k_loss_models constructs a probe's EpdNdf on the device, where no host value rides in the gamma slots: the
    # normalization takes float(tgamma(double(1 / p))) (epd.hpp EpdNdf()), while the eval entry points pass glibc's
    # tgammaf(1 / p) from the host (host_params<EpdM>), which is not correctly rounded.
    # At the golden sets' own p (0.2 and 1.886) the two agree and the sums are 0; at the scaled copies (p = 0.18,
    # 0.22, 2.074) tgammaf is an ulp off the correctly rounded float, and so is the normalization of every lane.
    "EPD",
}

# Rows whose last golden parameter set cannot give finite losses on 99 % of any pairs; they take the last set that
# can (the reference itself returns these values: tests/test_gpu_parity.py compares them NaN for NaN).
#   Ribardiere: sets 1 and 2 have gamma = 26.9 and 34.8; from gamma = 29.6 (set 1's third probe) the reference's eval
#     is NaN on a third of the pairs above the horizon, at 34.8 on every one of them.  Set 0 is left.
#   Bagher: set 2's Fresnel offsets F1 are all negative, eval is negative on a quarter of the pairs and
#     log(1 + eval cos) is NaN on 2-5 % of them.  Set 1 is finite.
LAST_FINITE_SET = {"Ribardiere": 0, "Bagher": 1}

ONE_HOT_ROWS = ["Lambertian", "CookTorrance", "Aggregate<Lambertian,Bagher>", "He"]
SMALL_N = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, N]
LARGE_N = 600_001
BATCH_ROWS = ["Lambertian", "CookTorrance", "Aggregate<Lambertian,Bagher>"]
NPROBES_BATCH = 1537             # 128 * 12 + 1: one more than the pair-major kernel's LDS rows allow
COMPONENT_SINGLES = ["Lambertian", "CookTorrance", "AshikhminShirleyFull"]     # diffuse, specular, both


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


@pytest.fixture(scope="module")
def merl(bbm, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("merl") / "synthetic.binary")
    ou.synthetic_merl(path)
    return bbm.Merl(path)


@pytest.fixture(scope="module")
def instances(bbm, merl):
    """As tests/test_gpu_image_models.py::instances: Merl over the synthetic table; the golden file's first and last
    parameter sets; the row's defaults where there is no golden data."""
    def make(name):
        if name == "Merl":
            return [merl]
        sets = [None]
        if name in META:
            g = ou.golden_model(name)
            last = LAST_FINITE_SET.get(name, len(META[name]["sets"]) - 1)
            sets = [g["params0"]] + ([g[f"params{last}"]] if last > 0 else [])
        out = []
        for p in sets:
            m = bbm.BsdfModel(name)
            if p is not None:
                m.set_parameter_values(p)
            out.append(m)
        return out
    return {name: make(name) for name in NAMES}


def with_params(m, p):
    """A copy of model m at parameters p (Merl: the model itself, its parameters are its table's address)."""
    if m.name == "Merl":
        assert np.array_equal(np.asarray(p, F).view(np.uint32), m.parameter_values().view(np.uint32))
        return m
    c = bbm_amd.BsdfModel(m.name)
    c.set_parameter_values(p)
    return c


def clipped(m, p):
    return np.clip(np.asarray(p, F), m.parameter_lower_bound(), m.parameter_upper_bound()).astype(F)


def probes_of(m):
    """The row's three probes: its parameters, and two copies scaled by 0.9 and 1.1 and clipped to the bounds -- three,
    so the two-probe unroll of k_loss_pairs has a remainder."""
    base = m.parameter_values()
    if m.name == "Merl":
        return np.stack([base, base, base])
    return np.stack([base, clipped(m, base * F(0.9)), clipped(m, base * F(1.1))])


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def staged_sum(kind, hin, hout, v, r):
    """(float64 sum of the per-sample losses, the per-sample losses): numpy float32 per sample, summed in double."""
    per = ou.np_loss(kind, hin, hout, v, r)
    return float(per.astype(np.float64).sum()), per


class Common:
    pass


@pytest.fixture(scope="module")
def common(bbm, instances):
    """The N pairs, the far tables, and per row and instance the probes and their staged evaluations (m.eval on the
    GPU).  N + SPARE candidate pairs are drawn; a pair at which any row's staged per-sample loss is not finite is
    dropped from the inputs (never masked out of a comparison), at most SPARE of them, and the first N of the rest
    are the inputs."""
    cand = N + SPARE
    din = bbm.fill_directions(SEED, 0, 0, cand, mode=0)          # upper hemisphere
    dout = bbm.fill_directions(SEED, 1, 0, cand, mode=1)         # whole sphere: below-horizon lanes included
    hin, hout = din.cpu().numpy(), dout.cpu().numpy()
    assert (hin[2] >= 0).all() and (hout[2] < 0).sum() > N // 4
    far = {False: bbm.GGX(roughness=0.2).eval(din, dout), True: bbm.CookTorrance(roughness=0.2).eval(din, dout)}
    hfar = {k: v.cpu().numpy() for k, v in far.items()}
    bad = np.zeros(cand, bool)
    for v in hfar.values():
        bad |= ~np.isfinite(v).all(0)
    rows = {}
    for name in NAMES:
        rows[name] = []
        for m in instances[name]:
            probes = probes_of(m)
            vals = np.stack([with_params(m, p).eval(din, dout).cpu().numpy() for p in probes])
            for v in vals:
                for kind in KINDS:
                    with np.errstate(all="ignore"):
                        bad |= ~np.isfinite(ou.np_loss(kind, hin, hout, v, hfar[name in GGX_ROWS]))
            rows[name].append((probes, vals))
    keep = np.nonzero(~bad)[0][:N]
    dropped = int(bad[:keep[-1] + 1].sum()) if keep.size else cand
    print(f"common inputs: {dropped} of the first {keep[-1] + 1 if keep.size else cand} candidate pairs dropped")
    assert keep.size == N and dropped <= SPARE, f"{int(bad.sum())} of {cand} candidate pairs are not finite for some row"
    c = Common()
    sel = torch.from_numpy(keep).cuda()
    c.din, c.dout = din[:, sel].contiguous(), dout[:, sel].contiguous()
    c.hin, c.hout = np.ascontiguousarray(hin[:, keep]), np.ascontiguousarray(hout[:, keep])
    c.far = {k: v[:, sel].contiguous() for k, v in far.items()}
    c.hfar = {k: np.ascontiguousarray(v[:, keep]) for k, v in hfar.items()}
    c.rows = {name: [(p, np.ascontiguousarray(v[:, :, keep])) for p, v in rows[name]] for name in NAMES}
    return c


def fused_sums(m, ref, kind, pairs, probes, component=3):
    from bbm_amd import fit
    loss = fit.SampledLoss(m, ref, kind, pairs=pairs, component=component)
    assert not loss.tree
    return loss.probe_sums(probes).cpu().numpy()


def tree_sums(m, ref, kind, pairs, probes, component=3):
    """bbm_hip_loss_tree on the one-leaf tree of a single model (bbm_amd.fit.SampledLoss takes the fused kernel for
    it): the probes through the eval entry point, the per-sample terms by k_loss_terms."""
    from bbm_amd.backbone import tree_desc
    lib = bbm_amd._lib.load()
    din, dout = pairs
    n = int(din.shape[1])
    p = np.ascontiguousarray(np.asarray(probes, F).reshape(-1, m.parameter_values().size))
    nprobes, npar = p.shape
    desc, nd, _keep = tree_desc(m)
    nbytes = lib.bbm_hip_loss_tree_workspace_size(nprobes, n)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device="cuda")
    sums = torch.full((nprobes,), float("nan"), dtype=torch.float64, device="cuda")
    bbm_amd._lib.check(lib.bbm_hip_loss_tree(desc, nd, p.ctypes.data, npar, nprobes, n, din[0].data_ptr(),
                                            din[1].data_ptr(), din[2].data_ptr(), dout[0].data_ptr(), dout[1].data_ptr(),
                                            dout[2].data_ptr(), ref[0].data_ptr(), ref[1].data_ptr(), ref[2].data_ptr(),
                                            int(kind), int(component), 0, sums.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                            torch.cuda.current_stream().cuda_stream))
    return sums.cpu().numpy()


def rel_dev(got, want):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got - want) / np.abs(want)
    d[got == want] = 0.0
    return float(np.max(d))


def test_all_rows_are_listed(bbm):
    assert len(NAMES) == 49 and len(set(NAMES)) == 49 and "Merl" in NAMES
    assert NOT_BITWISE <= set(NAMES) and GGX_ROWS <= set(NAMES) and len(AGGREGATES) == 14
    assert set(ONE_HOT_ROWS) | set(BATCH_ROWS) | set(COMPONENT_SINGLES) <= set(NAMES)
    assert not set(ONE_HOT_ROWS) & NOT_BITWISE


# ------------------------------------------------------------------------ 1. fused loss == staged pipeline

@pytest.mark.parametrize("name", NAMES)
def test_fused_loss_equals_staged_pipeline(bbm, instances, common, name):
    pairs, ref, href = (common.din, common.dout), common.far[name in GGX_ROWS], common.hfar[name in GGX_ROWS]
    worst = 0.0
    for m, (probes, vals) in zip(instances[name], common.rows[name]):
        for kind in KINDS:
            got = fused_sums(m, ref, kind, pairs, probes)
            want = []
            for v in vals:
                s, per = staged_sum(kind, common.hin, common.hout, v, href)
                assert np.isfinite(per).all(), (name, kind)
                want.append(s)
            want = np.asarray(want)
            assert (want > 0).all(), (name, kind, want)          # a far table: no probe is at the reference
            worst = max(worst, rel_dev(got, want))
            print(f"part 1 {name} kind {kind}: fused {got} staged {want} rel {rel_dev(got, want):.3e}")
            assert (np.abs(got - want) <= REL * np.abs(want)).all(), (name, kind, got, want)
    print(f"part 1 max rel deviation {name}: {worst:.3e}")


@pytest.mark.skipif(ou.ref() is None, reason="reference shim not built")
@pytest.mark.parametrize("kind", KINDS)
def test_fused_loss_equals_reference_losses(bbm, instances, common, kind):
    """The rows bbmref_loss accepts: the reference's own per-sample losses (sampledlossfunction over a table
    linearizer, oracle/ref_fit.cpp) between the probe and a second model of the same row (the parameters scaled by
    0.8), summed in double.  The GPU's reference table holds the reference's own eval of that second model, so both
    sides subtract the same values."""
    accepted = [n for n in NAMES if ou.ref_loss_accepts(n)]
    assert {"Aggregate<Lambertian,Bagher>", "Aggregate<Lambertian,CookTorrance>"} <= set(accepted), accepted
    worst = 0.0
    for name in accepted:
        for m, (probes, _vals) in zip(instances[name], common.rows[name]):
            second = clipped(m, m.parameter_values() * F(0.8))
            rv = ou.ref_eval_pdf(name, second, common.hin, common.hout, nthreads=8)[:3]
            assert np.isfinite(rv).all(), name
            got = fused_sums(m, torch.from_numpy(np.ascontiguousarray(rv)).cuda(), kind, (common.din, common.dout), probes)
            for p, g in zip(probes, got):
                per = ou.ref_pair_losses(name, p, second, common.hin, common.hout, kind)
                assert np.isfinite(per).all(), (name, kind)
                want = float(per.astype(np.float64).sum())
                worst = max(worst, rel_dev(g, want))
                print(f"part 1 (reference) {name} kind {kind}: fused {g} reference {want} rel {rel_dev(g, want):.3e}")
                assert want > 0 and abs(g - want) <= REL * abs(want), (name, kind, g, want)
    print(f"part 1 (reference) max rel deviation kind {kind}: {worst:.3e}")


# ------------------------------------------------------------------------ 2. fused loss == one-leaf tree path

@pytest.mark.parametrize("name", NAMES)
def test_fused_loss_equals_one_leaf_tree(bbm, instances, common, name):
    pairs, ref = (common.din, common.dout), common.far[name in GGX_ROWS]
    tol = REL if name in NOT_BITWISE else ORDER
    worst = 0.0
    for m, (probes, _vals) in zip(instances[name], common.rows[name]):
        for kind in KINDS:
            a = fused_sums(m, ref, kind, pairs, probes)
            b = tree_sums(m, ref, kind, pairs, probes)
            assert np.isfinite(a).all() and np.isfinite(b).all() and (b > 0).all(), (name, kind, a, b)
            worst = max(worst, rel_dev(a, b))
            np.testing.assert_allclose(a, b, rtol=tol, atol=0, err_msg=f"{name} kind {kind}")
    print(f"part 2 max rel deviation {name}: {worst:.3e}")


# ------------------------------------------------------------------------ 3. the loss's eval is the eval kernel's

@pytest.mark.parametrize("name", NAMES)
def test_own_eval_as_reference_gives_exact_zero(bbm, instances, common, name):
    """ref := the row's eval at a parameter vector and that vector among the probes: every per-sample error is v - v or
    log(1 + v c) - log(1 + v c) of the same floats, so all six sums of that probe are exactly 0.0 -- at the row's own
    parameters and at each of its two scaled copies, for every row outside NOT_BITWISE, and not everywhere for a row
    inside it (the list cannot grow or shrink silently)."""
    pairs = (common.din, common.dout)
    sums = []
    for m, (probes, _vals) in zip(instances[name], common.rows[name]):
        for j, p in enumerate(probes):
            ref = with_params(m, p).eval(*pairs)
            assert bool(torch.isfinite(ref).all()), name
            for kind in KINDS:
                s = fused_sums(m, ref, kind, pairs, probes)
                assert np.isfinite(s).all() and (s >= 0).all(), (name, kind, s)
                sums.append(float(s[j]))
    all_zero = all(s == 0.0 for s in sums)
    print(f"part 3 {name}: {'exactly 0' if all_zero else sums}")
    assert all_zero == (name not in NOT_BITWISE), (name, sums)


# ------------------------------------------------------------------------ 4. one-hot reference tables

def _one_hot_case(m, kind, din, dout, own, hin, hout, hown, indices):
    """For each index i: the reference table is the row's own eval except 2 ref + 0.5 at sample i, so every other
    sample adds exactly 0.0 and the sum over all n equals, bit for bit, the sum of a launch over pair i alone (views
    of length 1 into the same tensors); that launch against the staged value at REL."""
    from bbm_amd import fit
    n = int(din.shape[1])
    base = m.parameter_values()
    probes = np.stack([base, base, base])
    ref = own.clone()
    loss = fit.SampledLoss(m, ref, kind, pairs=(din, dout))
    zero = loss.local_sums(probes)
    whole, alone = [], []
    for i in indices:
        keep = ref[:, i].clone()
        ref[:, i] = 2.0 * keep + 0.5
        whole.append(loss.local_sums(probes))
        alone.append(loss.local_sums(probes, (din[:, i:i + 1], dout[:, i:i + 1]), ref[:, i:i + 1], 1))
        ref[:, i] = keep
    assert (zero.cpu().numpy() == 0.0).all(), (m.name, kind, n)
    whole, alone = torch.stack(whole).cpu().numpy(), torch.stack(alone).cpu().numpy()
    for k, i in enumerate(indices):
        hot = (F(2.0) * hown[:, i:i + 1] + F(0.5)).astype(F)
        want, _ = staged_sum(kind, hin[:, i:i + 1], hout[:, i:i + 1], hown[:, i:i + 1], hot)
        assert want > 0 and np.isfinite(want), (m.name, kind, n, i)
        assert (bits64(alone[k]) == bits64(alone[k][0])).all() and abs(alone[k][0] - want) <= REL * want, \
            (m.name, kind, n, i, alone[k], want)
        assert (bits64(whole[k]) == bits64(alone[k])).all(), (m.name, kind, n, i, whole[k], alone[k])


@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("name", ONE_HOT_ROWS)
def test_one_hot_reference_small_n(bbm, instances, common, name, kind):
    m = instances[name][0]
    own = m.eval(common.din, common.dout)
    hown = own.cpu().numpy()
    rng = np.random.default_rng(41)
    for n in SMALL_N:
        fixed = [i for i in (0, 1, 63, 64, 255, 256, 257, n - 2, n - 1) if 0 <= i < n]
        indices = sorted(set(fixed) | {int(i) for i in rng.integers(0, n, 8)})
        _one_hot_case(m, kind, common.din[:, :n], common.dout[:, :n], own[:, :n].contiguous(), common.hin[:, :n],
                      common.hout[:, :n], hown[:, :n], indices)


@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("name", ["Lambertian", "CookTorrance"])
def test_one_hot_reference_capped_grid(bbm, instances, name, kind):
    """n = 600 001: 2 344 workgroups of pairs, so the grid is capped at kLossMaxBlocks = 2 048, rounded down to whole
    device-fulls, and the workgroups' [lo, hi) shares differ in length."""
    n = LARGE_N
    assert (n + 255) // 256 > 2048 and n % 2048 != 0
    m = instances[name][0]
    din = bbm.fill_directions(SEED + 1, 0, 0, n, mode=0)
    dout = bbm.fill_directions(SEED + 1, 1, 0, n, mode=1)
    own = m.eval(din, dout)
    assert bool(torch.isfinite(own).all())
    rng = np.random.default_rng(43)
    indices = sorted({0, n - 1} | {int(i) for i in rng.integers(0, n, 64)})
    _one_hot_case(m, kind, din, dout, own, din.cpu().numpy(), dout.cpu().numpy(), own.cpu().numpy(), indices)


# ------------------------------------------------------------------------ 5. the probe-batch kernel

@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("name", BATCH_ROWS)
def test_probe_batch_kernel_equals_pair_major(bbm, instances, common, name, kind):
    """1537 probes need 4 x 1537 doubles of LDS in k_loss_pairs, more than launch_loss allows (48 KiB = 4 x 1536), so
    the launch takes k_loss (12 probes per pass); 1536 and 1 probes take k_loss_pairs.  Probes: the row's parameters
    (probe 0) and copies scaled per parameter by a factor in [0.8, 1.2], clipped to the bounds, fixed seed."""
    from bbm_amd import fit
    assert 4 * NPROBES_BATCH * 8 > 48 * 1024 >= 4 * (NPROBES_BATCH - 1) * 8
    m = instances[name][0]
    base = m.parameter_values()
    rng = np.random.default_rng(53)
    probes = np.stack([base] + [clipped(m, base * rng.uniform(0.8, 1.2, base.size).astype(F))
                                for _ in range(NPROBES_BATCH - 1)])
    ref, href = common.far[name in GGX_ROWS], common.hfar[name in GGX_ROWS]
    loss = fit.SampledLoss(m, ref, kind, pairs=(common.din, common.dout))
    batch = loss.local_sums(probes).cpu().numpy()
    split = np.concatenate([loss.local_sums(probes[:NPROBES_BATCH - 1]).cpu().numpy(),
                            loss.local_sums(probes[NPROBES_BATCH - 1:]).cpu().numpy()])
    assert batch.shape == split.shape == (NPROBES_BATCH,) and np.isfinite(batch).all() and (batch > 0).all()
    print(f"part 5 {name} kind {kind}: max rel deviation batch vs pair-major {rel_dev(batch, split):.3e}")
    np.testing.assert_allclose(batch, split, rtol=ORDER, atol=0)
    for j in (0, NPROBES_BATCH - 2, NPROBES_BATCH - 1):
        v = with_params(m, probes[j]).eval(common.din, common.dout).cpu().numpy()
        want, per = staged_sum(kind, common.hin, common.hout, v, href)
        assert np.isfinite(per).all() and abs(batch[j] - want) <= REL * abs(want), (name, kind, j, batch[j], want)


# ------------------------------------------------------------------------ 6. linearizer shards, n = 0

def _grid1():
    from bbm_amd import fit
    g = META_FIT["grids"]["grid1"]
    return fit.spherical_linearizer(g["samples_in"], g["samples_out"], g["start_in"], g["end_in"], g["start_out"],
                                    g["end_out"])


@pytest.mark.parametrize("kind", [0, 3])
@pytest.mark.parametrize("name", ["Aggregate<Lambertian,Bagher>", "CookTorrance"])
def test_in_kernel_linearizer_on_a_shard(bbm, instances, name, kind):
    """bbm_hip_loss computing the linearizer in-kernel over [begin, begin + n) == bbm_hip_loss_pairs over
    lin.directions(begin, n) with the same reference table, bit for bit: the four quarters of golden grid1 and 1217
    samples from 1 000 003 of the MERL grid.  The quarters' sums add up to the whole grid's."""
    from bbm_amd import fit
    m = instances[name][0]
    refm = bbm.GGX(roughness=0.2)
    probes = probes_of(m)
    g1, mg = _grid1(), fit.merl_linearizer()
    ranges = [(g1,) + fit.shard_range(g1.size(), r, 4) for r in range(4)] + [(mg, 1_000_003, 1_000_003 + N)]
    quarters = []
    for lin, b, e in ranges:
        n = e - b
        assert n % 256 != 0 and (b == 0 or b % 256 != 0) and e <= lin.size()
        loss = fit.SampledLoss(m, refm, kind, lin, materialize=False)
        assert loss.pairs is None and not loss.tree
        loss.begin, loss.n = b, n
        loss.ref = fit.reference_table(refm, lin, b, n)
        a = loss.local_sums(probes).cpu().numpy()
        pairs = lin.directions(b, n)
        c = loss.local_sums(probes, pairs, loss.ref, n).cpu().numpy()
        assert np.isfinite(a).all() and (a > 0).all(), (name, kind, b, n, a)
        assert (bits64(a) == bits64(c)).all(), (name, kind, b, n, a, c)
        if lin is g1:
            quarters.append(a)
    whole = fit.SampledLoss(m, refm, kind, g1, materialize=False).local_sums(probes).cpu().numpy()
    np.testing.assert_allclose(np.sum(quarters, axis=0), whole, rtol=ORDER, atol=0)


@pytest.mark.parametrize("name", ["Lambertian", "Aggregate<Lambertian,Bagher>", "He"])
def test_zero_samples(bbm, instances, name):
    """bbm_hip_loss and bbm_hip_loss_pairs called directly with n = 0 and valid workspaces (bbm_amd.fit returns zeros
    without a launch): BBM_HIP_OK, and every sum exactly 0.0 where the buffer held NaN."""
    lib = bbm_amd._lib.load()
    m = instances[name][0]
    p = np.ascontiguousarray(probes_of(m))
    nprobes, npar = p.shape
    dp = torch.from_numpy(p).cuda()
    ws = torch.empty(lib.bbm_hip_loss_workspace_size(nprobes) // 8, dtype=torch.float64, device="cuda")
    one = torch.zeros((9, 1), dtype=torch.float32, device="cuda")
    rows = [one[k].data_ptr() for k in range(9)]
    stream = torch.cuda.current_stream().cuda_stream
    lin = _grid1()
    for kind in (0, 3):
        for begin in (0, 378):
            sums = torch.full((nprobes,), float("nan"), dtype=torch.float64, device="cuda")
            rc = lib.bbm_hip_loss(m.model_id, dp.data_ptr(), npar, nprobes, ctypes.byref(lin), begin, 0, rows[6], rows[7],
                                  rows[8], kind, 3, 0, sums.data_ptr(), ws.data_ptr(), ws.numel() * 8, stream)
            assert rc == bbm_amd._lib.OK, lib.bbm_hip_last_error()
            assert (bits64(sums.cpu().numpy()) == 0).all(), (name, kind, begin, sums)
        sums = torch.full((nprobes,), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib.bbm_hip_loss_pairs(m.model_id, dp.data_ptr(), npar, nprobes, 0, *rows, kind, 3, 0, sums.data_ptr(),
                                    ws.data_ptr(), ws.numel() * 8, stream)
        assert rc == bbm_amd._lib.OK, lib.bbm_hip_last_error()
        assert (bits64(sums.cpu().numpy()) == 0).all(), (name, kind, sums)


# ------------------------------------------------------------------------ 7. components

@pytest.mark.parametrize("name", AGGREGATES + COMPONENT_SINGLES)
def test_components_reach_the_loss_kernels(bbm, instances, common, name):
    pairs, ref, href = (common.din, common.dout), common.far[name in GGX_ROWS], common.hfar[name in GGX_ROWS]
    flags = [bbm.bsdf_flag.Diffuse, bbm.bsdf_flag.Specular, bbm.bsdf_flag.All]
    for m, (probes, _vals) in zip(instances[name], common.rows[name]):
        for kind in (0, 3):
            got = {}
            for c in flags:
                got[c] = fused_sums(m, ref, kind, pairs, probes, component=int(c))
                for p, g in zip(probes, got[c]):
                    v = with_params(m, p).eval(*pairs, component=c).cpu().numpy()
                    want, per = staged_sum(kind, common.hin, common.hout, v, href)
                    assert np.isfinite(per).all() and want > 0, (name, kind, c)
                    assert abs(g - want) <= REL * abs(want), (name, kind, c, g, want)
            if name in AGGREGATES:
                d, s, a = (got[c][0] for c in flags)
                assert d != s and d != a and s != a, (name, kind, d, s, a)
