"""The edge ladder (tests/edge_params.py) checked with the reference alone, on the CPU: the conditions that keep
tests/test_gpu_edge_params.py from comparing zeros with zeros or from excusing every lane.

For every row of tests/golden/models.json, over all lanes of the row's ladder (sets x 224 lobe pairs, floatRGB
eval + pdf of the reference shim):
  (a) at least 40 % of the lanes have a normal finite reference value;
  (b) at least 30 % are well-conditioned (edge_params.classify) with a normal finite reference value;
  (c) every parameter of the row stands at its lo and at its hi* in some set.
"A normal finite reference value" is edge_params.normal_lanes: every channel finite, one at least >= FLT_MIN.
"""
import numpy as np
import pytest

from tests import edge_params as ep
from tests import oracle_util as ou

pytestmark = pytest.mark.skipif(ou.ref() is None, reason="oracle/_ref not built")

ROWS = list(ou.golden_meta()["models"])
MIN_NORMAL = 0.40
MIN_WELL_NORMAL = 0.30


def ladder_shares(name):
    """(lanes, share normal, share well-conditioned and normal, share ill-conditioned) of the row's ladder."""
    din, dout = ep.lobe_pairs()
    normal = well = ill = lanes = 0
    for _, p in ep.ladder(name):
        ref = ou.ref_eval_pdf(name, p, din, dout, nthreads=4)
        bad = ep.classify(lambda a, b: ou.ref_eval_pdf(name, p, a, b, nthreads=4), [din, dout], ref)
        nm = ep.normal_lanes(ref)
        lanes += nm.size
        normal += int(nm.sum())
        well += int((nm & ~bad).sum())
        ill += int(bad.sum())
    return lanes, normal / lanes, well / lanes, ill / lanes


def test_lobe_pairs_recipe():
    din, dout = ep.lobe_pairs()
    assert din.shape == dout.shape == (3, 224) and din.dtype == dout.dtype == np.float32
    for d in (din, dout):
        assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(0)) - 1).max() < 2e-7 and (d[2] >= 0).all()
    # lane 0: out = +z, delta = 0 -> in = out; the first block of 28 lanes shares one out
    assert (din[:, 0] == dout[:, 0]).all() and (dout[:, :28] == dout[:, :1]).all()
    assert sorted(set(np.round(dout[2].astype(np.float64), 6))) == [0.001, 0.1, 0.7, 1.0]
    # mirror lanes at delta = 0 are the mirror direction, retro lanes the out direction itself
    mirror0, retro0 = np.arange(0, 224, 28), np.arange(14, 224, 28)
    assert np.abs(din[:2, mirror0] + dout[:2, mirror0]).max() < 1e-7 and (din[:, retro0] == dout[:, retro0]).all()
    again = ep.lobe_pairs()
    assert (again[0] == din).all() and (again[1] == dout).all()


@pytest.mark.parametrize("name", ROWS)
def test_every_parameter_reaches_both_faces(name):
    _, lo, hi = ep.box(name)
    sets = ep.ladder(name)
    assert len({p.tobytes() for _, p in sets}) == len(sets)
    params = np.stack([p for _, p in sets])
    assert params.dtype == np.float32 and params.shape[1] == lo.size
    for j in range(lo.size):
        assert (params[:, j] == np.float32(lo[j])).any(), (name, j, "lo")
        assert (params[:, j] == np.float32(hi[j])).any(), (name, j, "hi*")
    faces = np.stack([p for _, p in ep.face_sets(name)])
    for j in range(lo.size):
        assert (faces[:, j] == np.float32(lo[j])).any() and (faces[:, j] == np.float32(hi[j])).any(), (name, j)
    assert all(len(g) > 1 and max(g) < lo.size for g in ep.attribute_groups(name))


@pytest.mark.parametrize("name", ROWS)
def test_ladder_is_not_vacuous(name):
    lanes, normal, well, ill = ladder_shares(name)
    print(f"{name}: {lanes} lanes, normal {normal:.3f}, well-conditioned and normal {well:.3f}, ill-conditioned {ill:.3f}")
    assert normal >= MIN_NORMAL, (name, normal)
    assert well >= MIN_WELL_NORMAL, (name, well)


def test_classify_is_seeded_and_uses_the_reference_alone():
    din, dout = ep.lobe_pairs()
    p = ep.ladder("CookTorrance")[0][1]
    fn = lambda a, b: ou.ref_eval_pdf("CookTorrance", p, a, b)
    ref = fn(din, dout)
    a, b = ep.classify(fn, [din, dout], ref), ep.classify(fn, [din, dout], ref)
    assert a.dtype == bool and a.shape == (224,) and (a == b).all()
    # a function that ignores its inputs has no ill-conditioned lane
    const =ep.classify(lambda a, b: np.tile(ref, (1, a.shape[1] // 224)), [din, dout], ref)
    assert not const.any()
