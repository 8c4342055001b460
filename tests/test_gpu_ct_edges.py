"""CookTorrance eval + pdf at the operands where a special-case select of a quotient or a root decides the result
(tests/ct_edge_lanes.py: z at 0, +-FLT_MIN, 1e-20 and 1, in == out, mirror pairs, halfway vectors with z(h) down to
1e-19, lower-hemisphere and masked lanes), for roughness and eta at both ends of their boxes and at the benchmark's
values, against the reference:
  * exact-subnormal mode: bit for bit on every lane;
  * default mode: the parity bar of oracle_util.parity_violations, no lane excused;
  * the four-pair kernel and the one-pair kernel (unaligned arrays) agree bit for bit in both modes.
N = 4 x 256 x 2 + 3 pairs: two full workgroups of quads and the scalar tail.  20 of the 2051 built lanes (0.98 %, the
limit is 20) are replaced by a plain pair because the reference itself is not finite there -- all of them pairs with
both z(in) and z(out) in (0, 1e-8], where z(in) z(out) or alpha^2 cos^4 underflows and the reference divides 0 by 0
or overflows: 7 of the 9 quarter-turn grazing pairs with equal z (z(h) from 1e-8 down to 1e-19; the two at 1e-3 and
1e-5 and all 9 paired with z = 1e-3 stay), in == out at z = 1e-8, 1e-19, 1e-20, 1e-30 and FLT_MIN, the mirror pairs at
z = 1e-19, 1e-20, 1e-30 and FLT_MIN, and the four combinations of z in {FLT_MIN, 1e-20}.  Every lane with a z of 0,
-FLT_MIN or 1 stays, as do in == out and the mirror pairs down to z = 1e-3 and 1e-8.
"""
import numpy as np
import pytest
import torch

from tests import ct_edge_lanes as ce
from tests import oracle_util as ou

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bbm():
    import bbm_amd
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eval(model, din, dout, exact, mask=None):
    rgb, pdf = model.eval_pdf(din, dout, mask=mask, exact=exact)
    torch.cuda.synchronize()
    return np.concatenate([rgb.cpu().numpy(), pdf.cpu().numpy()[None]], 0)


def _unaligned(a):
    """The same rows one float into a larger buffer: 4-byte-aligned pointers, which take the one-pair kernel."""
    buf = torch.empty((a.shape[0], a.shape[1] + 1), dtype=a.dtype, device=a.device)
    buf[:, 1:] = a
    return tuple(buf[i, 1:] for i in range(a.shape[0]))


def test_reference_is_finite_on_the_lanes():
    assert ou.ref() is not None, "oracle/_ref/libbbm_ref.so is missing: these tests compare against the reference"
    _, _, refs, dropped = ce.lanes()
    assert dropped <= ce.N // 100, dropped
    assert len(refs) == 9


@pytest.mark.parametrize("tag", [t for t, _ in ce.param_sets()])
def test_edges_against_reference(bbm, tag):
    assert ou.ref() is not None, "oracle/_ref/libbbm_ref.so is missing: these tests compare against the reference"
    din, dout, refs, _ = ce.lanes()
    params = dict(ce.param_sets())[tag]
    ref = refs[tag]
    m = bbm.BsdfModel(ce.NAME)
    m.set_parameter_values(params)
    di, do = torch.from_numpy(din.copy()).cuda(), torch.from_numpy(dout.copy()).cuda()
    mk_host = ce.mask()
    mk = torch.from_numpy(mk_host).cuda()
    ref_masked = np.where(mk_host[None] != 0, ref, np.float32(0))
    for exact in (True, False):
        quad = _eval(m, di, do, exact)
        one = _eval(m, _unaligned(di), _unaligned(do), exact)
        quad_m = _eval(m, di, do, exact, mask=mk)
        one_m = _eval(m, _unaligned(di), _unaligned(do), exact, mask=_unaligned(mk[None])[0])
        diff = np.nonzero(_bits(quad) != _bits(one))
        print(f"{tag} exact={exact}: quad vs one-pair differing values {diff[0].size}")
        assert diff[0].size == 0, (tag, exact, diff[1][:8])
        assert np.array_equal(_bits(quad_m), _bits(one_m)), (tag, exact)
        live = mk_host != 0
        assert np.array_equal(_bits(quad_m)[:, live], _bits(quad)[:, live]), (tag, exact)
        assert not quad_m[:, ~live].any(), (tag, exact)
        for got, want, what in ((quad, ref, "all"), (quad_m, ref_masked, "masked")):
            if exact:
                bad = np.nonzero(_bits(got) != _bits(want))
                print(f"{tag} exact {what}: values differing from the reference {bad[0].size} of {got.size}")
                assert bad[0].size == 0, (tag, what, bad[1][:8], got[bad][:8], want[bad][:8],
                                          din[:, bad[1][:4]].T, dout[:, bad[1][:4]].T)
            else:
                bad = ou.parity_violations(got, want)
                print(f"{tag} default {what}: lanes outside the parity bar {bad[0].size}, bit-identical "
                      f"{float(np.mean(_bits(got) == _bits(want))):.5f}")
                assert bad[0].size == 0, (tag, what, bad[1][:8], got[bad][:8], want[bad][:8])
