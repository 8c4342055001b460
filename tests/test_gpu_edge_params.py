"""Every registry row at the faces of its parameter box, on directions aimed at the lobe (GPU; -m gpu).

The parity tests of tests/test_gpu_parity.py run parameters from the middle of each box on directions that almost
never land in a sharp lobe.  Here the parameter sets are tests/edge_params.ladder (each parameter at lo, hi* and
three steps next to lo, attributes moved as a whole, both corners) and the 224 pairs are edge_params.lobe_pairs
(within 0 .. 0.5 of the mirror and the retro direction).  tests/test_edge_params_host.py holds the same lane set to
its conditions with the reference alone.

The reference is sensitive to the last bit of its inputs at these parameters, so every lane is classified from the
reference side (edge_params.classify) before the GPU value is looked at:
  * well-conditioned lanes go through test_gpu_parity.check_lanes as the 1 M-pair test applies it (the bar, the
    provers, the caps on how many lanes may need a proof and by how much), set by set;
  * ill-conditioned lanes must each meet the bar or be proven by the input-ulps prover (<= 4 float steps); none is
    dropped, their number is bounded from the reference side by the host test's condition (b).

  1. eval_pdf floatRGB per set against the reference;            4. exact mode on the Beckmann rows;
  2. doubleRGB per set against the reference's doubleRGB;         5. varying= rows, a MaterialTable and sample_eval
  3. sample and reflectance at the faces and the corners;            against the uniform calls, bit for bit.
Statistics: parity_edge_<what>.json, written by test_gpu_parity._report next to its other reports.
"""
import numpy as np
import pytest

import bbm_amd
from tests import edge_params as ep
from tests import oracle_util as ou
from tests.test_gpu_parity import (_check_samples, _evalpdf_provers, _gpu_sample, _input_ulps_prover, _report,
                                   check_lanes)
from tests.test_gpu_table import SIZE_ROWS

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(ou.ref() is None, reason="oracle/_ref not built")]

F = np.float32
META = ou.golden_meta()["models"]
ROWS = [n for n in bbm_amd.model_names() if n in META]
F64_ROWS = [n for n in ROWS if bbm_amd.BsdfModel(n).has_f64()]
BECKMANN_ROWS = ["CookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "LowCookTorrance", "NganCookTorrance"]
LANE_ROWS = list(dict.fromkeys(SIZE_ROWS + ["He", "EPD"]))
DIN, DOUT = ep.lobe_pairs()
EDGE_SAMPLES = 50                 # the golden sample inputs' edge block: xi on the clamps, grazing views
INP = ou.golden_inputs()
SOUT = np.ascontiguousarray(INP["sout"][:, -EDGE_SAMPLES:])
SXI = np.ascontiguousarray(INP["sxi"][:, -EDGE_SAMPLES:])


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


def _tag(name):
    return name.replace("<", "_").replace(",", "_").replace(">", "")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).astype(dtype))).cuda()


def model_at(name, p):
    m = bbm_amd.BsdfModel(name)
    m.set_parameter_values(np.asarray(p, F))
    return m


def _evalpdf(m, dtype=np.float32, **kw):
    rgb, pdf = m.eval_pdf(_dev(DIN, dtype), _dev(DOUT, dtype), **kw)
    torch.cuda.synchronize()
    return np.concatenate([rgb.cpu().numpy(), pdf.cpu().numpy()[None]], 0)


def test_rows_are_listed(bbm):
    assert len(ROWS) == 48 and set(BECKMANN_ROWS) | set(LANE_ROWS) <= set(ROWS) and len(F64_ROWS) >= 37


# ------------------------------------------------------------------------ 1, 4. eval_pdf floatRGB

def _ladder_f32(bbm, name, what):
    """The row's ladder through eval_pdf floatRGB, set by set, in the process's current mode -> statistics."""
    st = {"sets": 0, "lanes": 0, "ill_conditioned": 0, "lanes_outside_bar": 0, "ill_outside_bar": 0, "proven_by": {},
          "max_rel_normal": 0.0, "max_rel_normal_well": 0.0, "bit_exact": 0, "normal_lanes": 0}
    for tag, p in ep.ladder(name):
        got = _evalpdf(model_at(name, p))
        ref = ou.ref_eval_pdf(name, p, DIN, DOUT, nthreads=8)
        ill = ep.classify(lambda a, b: ou.ref_eval_pdf(name, p, a, b, nthreads=8), [DIN, DOUT], ref)
        w, i = np.nonzero(~ill)[0], np.nonzero(ill)[0]
        s = check_lanes(got[:, w], ref[:, w], f"{name} {what} {tag} well-conditioned",
                        _evalpdf_provers(bbm, name, p, DIN[:, w], DOUT[:, w], got[:, w]), model=name)
        # ill-conditioned lanes: the bar, or the reference's own values at inputs <= 4 float steps away bracket the GPU's
        bad = i[~ou.parity_ok(got[:, i], ref[:, i]).all(0)]
        if bad.size:
            prove = _input_ulps_prover(lambda a, b: ou.ref_eval_pdf(name, p, a, b, nthreads=8), [DIN, DOUT], got)
            left = bad[~prove(bad)]
            assert left.size == 0, (f"{name} {what} {tag}: {left.size} ill-conditioned lanes outside the bar and not "
                                    f"bracketed by the reference at inputs <= 4 float steps away; lanes {left[:4]}: "
                                    f"got {got[:, left[:4]].T.tolist()} ref {ref[:, left[:4]].T.tolist()}")
            st["proven_by"]["input_ulps_ill"] = st["proven_by"].get("input_ulps_ill", 0) + int(bad.size)
        for k, v in s["proven_by"].items():
            st["proven_by"][k] = st["proven_by"].get(k, 0) + v
        st["sets"] += 1
        st["lanes"] += DIN.shape[1]
        st["ill_conditioned"] += int(ill.sum())
        st["lanes_outside_bar"] += s["lanes_outside_bar"] + int(bad.size)
        st["ill_outside_bar"] += int(bad.size)
        st["max_rel_normal"] = max(st["max_rel_normal"], ou.max_rel_normal(got, ref))
        st["max_rel_normal_well"] = max(st["max_rel_normal_well"], s["max_rel_normal"])
        st["bit_exact"] += int((ou.ulp_diff(got, ref) == 0).all(0).sum())
        st["normal_lanes"] += int(ep.normal_lanes(ref).sum())
    st["ill_conditioned_share"] = st["ill_conditioned"] / st["lanes"]
    st["frac_bit_exact"] = st.pop("bit_exact") / st["lanes"]
    st["normal_share"] = st.pop("normal_lanes") / st["lanes"]
    return st


@pytest.mark.parametrize("name", ROWS)
def test_eval_pdf_at_the_box_faces(bbm, name):
    _report(f"edge_f32_{_tag(name)}", _ladder_f32(bbm, name, "f32"))


@pytest.mark.parametrize("name", BECKMANN_ROWS)
def test_exact_mode_at_the_box_faces(bbm, name):
    """bbm_hip_set_exact_subnormals(1): the same bar; the bit-identical fraction is reported, not asserted."""
    assert bbm.set_exact_subnormals(True) is False
    try:
        st = _ladder_f32(bbm, name, "exact")
    finally:
        bbm.set_exact_subnormals(False)
    _report(f"edge_exact_{_tag(name)}", st)


# ------------------------------------------------------------------------ 2. doubleRGB

@pytest.mark.parametrize("name", F64_ROWS)
def test_f64_eval_pdf_at_the_box_faces(bbm, name):
    """Both classes: the bar (oracle_util.parity_ok_f64) or the input-ulps bracket of the double reference -- <= 2
    float steps and at most max(2, 1e-3 n) lanes a set for the well-conditioned lanes, <= 4 for the others."""
    st = {"sets": 0, "lanes": 0, "ill_conditioned": 0, "lanes_outside_bar": 0, "proven_input_ulps": 0,
          "max_rel_normal": 0.0, "max_rel_normal_well": 0.0}
    n = DIN.shape[1]
    for tag, p in ep.ladder(name):
        fn = lambda a, b: ou.ref_eval_pdf_double(name, p, a, b, nthreads=8)
        got = _evalpdf(model_at(name, p), np.float64)
        assert got.dtype == np.float64
        ref = fn(DIN, DOUT)
        ill = ep.classify(fn, [DIN, DOUT], ref, ok=ou.parity_ok_f64)
        bad = np.nonzero(~ou.parity_ok_f64(got, ref).all(0))[0]
        for lanes, k, trials, cap in ((bad[~ill[bad]], 2, 48, max(2, 1e-3 * n)), (bad[ill[bad]], 4, 128, n)):
            if lanes.size == 0:
                continue
            ok = ou.explained_by_input_ulps(fn, [DIN[:, lanes], DOUT[:, lanes]], got[:, lanes], k=k, trials=trials)
            left = lanes[~ok]
            assert left.size == 0, (f"{name} f64 {tag}: {left.size} lanes outside the 1e-5 bar and not proven "
                                    f"(<= {k} float steps); lanes {left[:4]}: got {got[:, left[:4]].T.tolist()} "
                                    f"ref {ref[:, left[:4]].T.tolist()}")
            assert lanes.size <= cap, f"{name} f64 {tag}: {lanes.size} well-conditioned lanes needed a proof"
            st["proven_input_ulps"] += int(lanes.size)
        err = ou.rel_err_f64(got, ref)
        sel = (np.abs(ref) >= ou.DBL_MIN) & np.isfinite(ref)
        st["sets"] += 1
        st["lanes"] += n
        st["ill_conditioned"] += int(ill.sum())
        st["lanes_outside_bar"] += int(bad.size)
        st["max_rel_normal"] = max(st["max_rel_normal"], float(err[sel].max()) if sel.any() else 0.0)
        well = sel & ~ill[None]
        st["max_rel_normal_well"] = max(st["max_rel_normal_well"], float(err[well].max()) if well.any() else 0.0)
    st["ill_conditioned_share"] = st["ill_conditioned"] / st["lanes"]
    _report(f"edge_f64_{_tag(name)}", st)


# ------------------------------------------------------------------------ 3. sample and reflectance

@pytest.mark.parametrize("name", ROWS)
def test_sample_and_reflectance_at_the_box_faces(bbm, name):
    stats = {}
    for tag, p in ep.face_sets(name):
        m = model_at(name, p)
        got, flag = _gpu_sample(m, SOUT, SXI)
        ref, rflag = ou.ref_sample(name, p, SOUT, SXI, nthreads=8)
        s = _check_samples(bbm, name, p, SOUT, SXI, got, flag, ref, rflag, f"{name} {tag}")
        refl = m.reflectance(_dev(SOUT)).cpu().numpy()
        prove = _input_ulps_prover(lambda o: ou.ref_reflectance(name, p, o), [SOUT], refl)
        r = check_lanes(refl, ou.ref_reflectance(name, p, SOUT), f"{name} {tag} reflectance", [prove], model=name)
        stats[tag] = {"sample_pdf_lanes_outside_bar": s["lanes_outside_bar"], "sample_pdf_proven_by": s["proven_by"],
                      "sample_pdf_max_rel_normal": s["max_rel_normal"], "dir_lanes_outside_bar": s["dir_lanes_outside_bar"],
                      "dir_proven_by": s["dir_proven_by"], "max_dir_abs_err": s["max_dir_abs_err"],
                      "reflectance_lanes_outside_bar": r["lanes_outside_bar"], "reflectance_proven_by": r["proven_by"],
                      "reflectance_max_rel_normal": r["max_rel_normal"], "reflectance_frac_bit_exact": r["frac_bit_exact"]}
    _report(f"edge_sample_{_tag(name)}", stats)


# ------------------------------------------------------------------------ 5. the per-lane sources

def i32(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.int32)


def run(m, din, dout, xi, **kw):
    """eval_pdf, reflectance and sample of one call as (12, n) bits."""
    rgb, pdf = m.eval_pdf(din, dout, **kw)
    refl = m.reflectance(dout, **kw)
    s = m.sample(dout, xi, **kw)
    return np.concatenate([i32(rgb), i32(pdf)[None], i32(refl), i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None]])


def same(got, want, what):
    diff = np.nonzero((got != want).any(0))[0]
    assert diff.size == 0, (what, f"{diff.size} lanes differ", diff[:8], got[:, diff[:2]], want[:, diff[:2]])


@pytest.mark.parametrize("name", LANE_ROWS)
def test_per_lane_sources_at_the_box_faces(bbm, name):
    """Lane i carries the ladder's set i mod K, as varying= rows and as a MaterialTable's material: each lane equals
    the uniform call at its set, bit for bit (EPD's varying lanes whose p is not the call's uniform p: the parity bar,
    its normalization's tgamma).  n = 224 K + 1 lanes: lane i is lobe pair (i div K) mod 224, so every
    set meets every pair, and the odd lane takes the scalar tail; xi from the library's generator.  The uniform call of
    set k runs on that set's lanes alone (the kernels are per-pair independent).  sample_eval at the two corners
    equals its staged sample / eval_pdf calls and the float32 weight rule.  A row without per-lane kernels (He) must
    say so."""
    from bbm_amd.plot import plot_draws
    sets = np.stack([p for _, p in ep.ladder(name)])
    K = len(sets)
    n = 224 * K + 1
    lane = np.arange(n)
    pair, assign = (lane // K) % 224, lane % K
    din, dout, xi = _dev(DIN[:, pair]), _dev(DOUT[:, pair]), plot_draws(0xED6E, 0, n)
    m = model_at(name, sets[0])
    stats = {"sets": K, "lanes": n}
    if m.has_varying() or m.has_table():
        assert m.has_varying() and m.has_table()
        want = np.zeros((12, n), np.int32)
        for k in range(K):
            idx = torch.from_numpy(np.nonzero(assign == k)[0]).cuda()
            want[:, assign == k] = run(model_at(name, sets[k]), din[:, idx].contiguous(), dout[:, idx].contiguous(),
                                       xi[:, idx].contiguous())
        rows = torch.from_numpy(np.ascontiguousarray(sets[assign].T)).cuda()
        got_v = run(m, din, dout, xi, varying={k: rows[k] for k in range(rows.shape[0])})
        t = bbm.MaterialTable(name, sets)
        got_t = run(t, din, dout, xi, material=torch.from_numpy(assign.astype(np.int32)).cuda())
        t.close()
        same(got_t, want, (name, "table"))
        if name == "EPD":
            host_p = sets[assign, 1] == sets[0, 1]
            same(got_v[:, host_p], want[:, host_p], (name, "varying, the uniform p"))
            gf, wf = got_v[:11].view(F), want[:11].view(F)
            bad = ou.parity_violations(gf, wf)
            assert bad[0].size == 0 and (got_v[11] == want[11]).all(), (name, "varying", bad)
            stats["varying_lanes_not_bit_identical"] = int((got_v != want).any(0).sum())
        else:
            same(got_v, want, (name, "varying"))
    else:
        for call in (lambda: m.eval_pdf(din, dout, varying={}), lambda: bbm.MaterialTable(name, sets)):
            with pytest.raises(bbm._lib.BackboneError) as e:
                call()
            assert e.value.code == bbm._lib.ERR_UNSUPPORTED
        stats["per_lane_kernels"] = False
    eps = F(np.finfo(np.float32).eps)
    for tag, p in ep.corner_sets(name):
        mc = model_at(name, p)
        s, v, w = mc.sample_eval(dout, xi)
        s2 = mc.sample(dout, xi)
        v2, _ = mc.eval_pdf(s2.direction, dout)
        fused = np.concatenate([i32(s.direction), i32(s.pdf)[None], i32(s.flag)[None], i32(v)])
        staged = np.concatenate([i32(s2.direction), i32(s2.pdf)[None], i32(s2.flag)[None], i32(v2)])
        nan = np.isnan(fused[:4].view(F)), np.isnan(staged[:4].view(F))        # NaN lanes by place, not by payload
        assert (nan[0] == nan[1]).all(), (name, tag, "NaN lanes differ")
        vn = np.isnan(fused[5:].view(F)), np.isnan(staged[5:].view(F))
        assert (vn[0] == vn[1]).all(), (name, tag, "NaN values differ")
        fused[:4][nan[0]] = staged[:4][nan[1]] = 0
        fused[5:][vn[0]] = staged[5:][vn[1]] = 0
        same(fused, staged, (name, tag, "sample_eval against its staged calls"))
        hv, hw, hp, hz = v.cpu().numpy(), w.cpu().numpy(), s.pdf.cpu().numpy()[None], s.direction[2].cpu().numpy()[None]
        with np.errstate(all="ignore"):
            rule = np.where(np.broadcast_to(hp > eps, hv.shape), ((hv * hz).astype(F) / hp).astype(F), F(0)).astype(F)
        wn = np.isnan(hw)
        assert (wn == np.isnan(rule)).all() and (np.where(wn, F(0), hw).view(np.int32) ==
                                                 np.where(wn, F(0), rule).view(np.int32)).all(), (name, tag, "weight")
        stats[f"sample_eval {tag}"] = {"finite_weight_lanes": int(np.isfinite(hw).all(0).sum())}
    _report(f"edge_lanes_{_tag(name)}", stats)
