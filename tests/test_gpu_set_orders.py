"""The two orders of the material-set calls are one call: a call in lane order (bbm_hip_set_eval_pdf,
bbm_hip_set_sample_eval and their _tangent forms) is the call in plan order (the _sorted forms) between a gather into
scratch and a scatter out of it, behind the same checks in the same order.

  1. a bad argument set is refused with the same code and message in both orders, the earlier fault first, and no
     output is written; the messages are the literals below, not read from the library's source;
  2. lane order == plan.scatter(plan order(plan.gather(...))) bit for bit on the live lanes, at the most and the fewest
     streams a lane-order call moves through its scratch.

A three-table set with one anisotropic row and 67 lanes: no multiple of four, so every segment ends in padding; the
ids leave the middle row empty and some are out of range; the mask has dead lanes.
"""
import ctypes

import numpy as np
import pytest

import bbm_amd

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
SEED = 0x0DE5
N = 67
ROWS = ["Lambertian", "CookTorrance", "Ward"]              # Ward: the anisotropic row
ISOTROPIC = ["Lambertian", "CookTorrance", "GGX"]
SIZES = (3, 4, 3)


def table_of(name, count):
    m = bbm_amd.BsdfModel(name)
    scale = np.linspace(0.6, 1.0, count, dtype=F)[:, None]
    params = np.clip(m.parameter_values()[None] * scale, m.parameter_lower_bound(), m.parameter_upper_bound())
    return bbm_amd.MaterialTable(name, params.astype(F))


def bits(*ts):
    """Tensors (1-D or (k, n)) as one (rows, n) int32 CUDA tensor of bit patterns."""
    return torch.cat([(t if t.dim() == 2 else t[None]).contiguous().view(torch.int32) for t in ts if t is not None])


class Batch:
    pass


@pytest.fixture(scope="module")
def batch():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    from bbm_amd.plot import plot_draws
    c = Batch()
    rng = np.random.default_rng(SEED)
    c.mset = bbm_amd.MaterialSet([table_of(name, m) for name, m in zip(ROWS, SIZES)])
    c.isotropic = bbm_amd.MaterialSet([table_of(name, m) for name, m in zip(ISOTROPIC, SIZES)])
    assert c.mset.offsets == c.isotropic.offsets == [0, 3, 7, 10]
    ids = np.where(rng.random(N) < 0.5, rng.integers(0, 3, N), rng.integers(7, 10, N))      # the middle row stays empty
    ids[5::23] = -1                                                                          # out of range: row 0's
    c.ids = torch.from_numpy(ids.astype(np.int32)).cuda()
    c.plan = c.mset.plan(c.ids)
    c.iso_plan = c.isotropic.plan(c.ids)
    seg = c.plan.segments
    assert seg[1] == seg[2] and seg[0] < seg[1] and seg[2] < seg[3], seg
    assert c.plan.capacity > N and c.iso_plan.segments == seg
    c.din = bbm_amd.fill_directions(SEED, 0, 0, N, mode=1)
    c.dout = bbm_amd.fill_directions(SEED, 1, 0, N, mode=1)
    c.xi = plot_draws(SEED, 0, N)
    normal = rng.normal(size=(3, N)).astype(F) * rng.uniform(0.1, 3.0, N).astype(F)
    normal[:, 7::31] = 0                      # normals that are not live
    c.normal = torch.from_numpy(normal).cuda()
    tangent = rng.normal(size=(3, N)).astype(F)
    tangent[:, 3::29] = 0                     # tangents that fall back to the normal's frame
    c.tangent = torch.from_numpy(tangent).cuda()
    mask = (rng.random(N) < 0.8).astype(np.uint8)
    assert 0 < mask.sum() < N
    c.mask = torch.from_numpy(mask).cuda()
    return c


# ------------------------------------------------------------------------ 1. the same refusals in both orders

EVAL_PDF, SAMPLE_EVAL = "eval_pdf", "sample_eval"
TANGENT = b"tangent: give tx, ty and tz or none"
COMPACT = b"a compact plan leaves lanes out: use the calls in plan order (the *_sorted calls)"
PLAN = b"plan is NULL"
FLAGS = b"call_flags must be 0, BBM_HIP_CALL_EXACT or BBM_HIP_CALL_DEFAULT"
LENGTH = {"lanes": b"n is %d, the plan was made for %d lanes", "plan": b"slots is %d, the plan's capacity is %d"}
NORMAL = b"normal: give nx, ny and nz or none"
TANGENT_NORMAL = b"tangent needs a normal: it fills the frame of the world-space call"
COS_NORMAL = b"cos_in needs a normal: it is the cosine of `in` against it"
NO_OUTPUT = b"every output pointer is NULL"
PARTIAL_RGB = b"eval output pointer is NULL"
PARTIAL_VALUE = b"value output: give r, g and b or none"
PARTIAL_WEIGHT = b"weight output: give wr, wg and wb or none"
XI = b"xi pointer is NULL"
SAMPLE_OUTPUT = b"sample output pointer is NULL"

# (what, the call kinds it applies to, the arguments that differ from a good call, the message).  Arguments: plan
# (False: NULL, or another plan's handle), flags, normal / tangent (which of the three pointers are given), length (added to the right one),
# and per kind rgb / pdf / cos, or xi / req / value / weight (which pointers are given).
NO3, ALL3 = (False,) * 3, (True,) * 3
BOTH = (EVAL_PDF, SAMPLE_EVAL)
BAD_FLAGS = 0x30000000                         # BBM_HIP_CALL_EXACT | BBM_HIP_CALL_DEFAULT
REFUSED = [
    ("mixed tangent", BOTH, dict(tangent=(True, False, False)), TANGENT),
    ("mixed tangent, its last alone", BOTH, dict(tangent=(False, False, True)), TANGENT),
    ("mixed normal", BOTH, dict(normal=(True, False, True)), NORMAL),
    ("tangent without normal", BOTH, dict(normal=NO3, tangent=ALL3, cos=False), TANGENT_NORMAL),
    ("cos_in without normal", (EVAL_PDF,), dict(normal=NO3), COS_NORMAL),
    ("every output NULL", (EVAL_PDF,), dict(rgb=NO3, pdf=False, cos=False), NO_OUTPUT),
    ("partial rgb", (EVAL_PDF,), dict(rgb=(True, False, True)), PARTIAL_RGB),
    ("partial value", (SAMPLE_EVAL,), dict(value=(True, False, False)), PARTIAL_VALUE),
    ("partial weight", (SAMPLE_EVAL,), dict(weight=(False, True, False)), PARTIAL_WEIGHT),
    ("NULL xi1", (SAMPLE_EVAL,), dict(xi=(True, False)), XI),
    ("NULL sample output", (SAMPLE_EVAL,), dict(req=(True, True, True, False, True)), SAMPLE_OUTPUT),
    ("NULL flag", (SAMPLE_EVAL,), dict(req=(True, True, True, True, False)), SAMPLE_OUTPUT),
    ("bad flags", BOTH, dict(flags=BAD_FLAGS), FLAGS),
    ("unknown flag", BOTH, dict(flags=1), FLAGS),
    ("wrong length", BOTH, dict(length=4), LENGTH),
    ("length 0", BOTH, dict(length=None), LENGTH),
    ("NULL plan", BOTH, dict(plan=False), PLAN),
    # two faults at once: the earlier check wins
    ("tangent mixture + NULL plan", BOTH, dict(tangent=(False, True, False), plan=False), TANGENT),
    ("NULL plan + bad flags", BOTH, dict(plan=False, flags=BAD_FLAGS), PLAN),
    ("bad flags + wrong length", BOTH, dict(flags=BAD_FLAGS, length=4), FLAGS),
    ("wrong length + mixed normal", BOTH, dict(length=-4, normal=(False, True, True)), LENGTH),
    ("mixed normal + tangent", BOTH, dict(normal=(True, True, False), tangent=ALL3), NORMAL),
    ("mixed normal + NULL output", (EVAL_PDF,), dict(normal=(False, False, True), rgb=NO3, pdf=False, cos=False), NORMAL),
    ("mixed normal + NULL output", (SAMPLE_EVAL,), dict(normal=(False, False, True), req=(False,) * 5), NORMAL),
    ("tangent and cos_in without normal", (EVAL_PDF,), dict(normal=NO3, tangent=ALL3), TANGENT_NORMAL),
    ("cos_in without normal + partial rgb", (EVAL_PDF,), dict(normal=NO3, rgb=(False, True, True)), COS_NORMAL),
    ("tangent without normal + NULL xi", (SAMPLE_EVAL,), dict(normal=NO3, tangent=ALL3, xi=(False, False)), TANGENT_NORMAL),
    ("NULL xi + partial value", (SAMPLE_EVAL,), dict(xi=(False, True), value=(False, False, True)), XI),
    ("NULL sample output + partial weight", (SAMPLE_EVAL,), dict(req=(False,) + (True,) * 4, weight=(True, True, False)),
     SAMPLE_OUTPUT),
    ("partial value + partial weight", (SAMPLE_EVAL,), dict(value=(False, True, True), weight=(True, False, True)),
     PARTIAL_VALUE),
]
STAMP = 123.0


def test_the_same_refusals_in_both_orders(batch):
    c = batch
    lib, L = bbm_amd._lib.load(), bbm_amd._lib
    cap = c.plan.capacity
    lengths = {"lanes": N, "plan": cap}
    rows = lambda t: [ctypes.c_void_p(t[k].data_ptr()) for k in range(t.shape[0])]
    some = lambda ptrs, given: [p if g else None for p, g in zip(ptrs, given)]
    # the streams of a good call in each order; a refused call reads none of them
    streams, outs = {}, {}
    for order, count in lengths.items():
        g = torch.Generator(device="cuda")
        g.manual_seed(SEED)
        streams[order] = {k: rows(torch.rand((r, count), device="cuda", generator=g))
                          for k, r in (("normal", 3), ("tangent", 3), ("in", 3), ("out", 3), ("xi", 2))}
        streams[order]["keep"] = torch.ones((count,), dtype=torch.uint8, device="cuda")
        outs[order] = torch.full((16, count), STAMP, device="cuda")

    def call(kind, order, form, plan=True, flags=0, normal=ALL3, tangent=NO3, length=0, rgb=ALL3, pdf=True, cos=True,
             xi=(True, True), req=(True,) * 5, value=NO3, weight=ALL3):
        s, o = streams[order], rows(outs[order])
        handle = None if plan is False else c.plan._handle if plan is True else plan
        frame = some(s["normal"], normal) + (some(s["tangent"], tangent) if form != "plain" else [])
        count = 0 if length is None else lengths[order] + length
        mask = ctypes.c_void_p(s["keep"].data_ptr())
        if kind == EVAL_PDF:
            fn = {"plain": lib.bbm_hip_set_eval_pdf, "tangent": lib.bbm_hip_set_eval_pdf_tangent,
                  "sorted": lib.bbm_hip_set_eval_pdf_sorted}[form]
            rc = fn(handle, flags, *frame, *s["in"], *s["out"], mask, count, 3, 0, *some(o[:3], rgb),
                    *some(o[3:5], (pdf, cos)), None)
        else:
            fn = {"plain": lib.bbm_hip_set_sample_eval, "tangent": lib.bbm_hip_set_sample_eval_tangent,
                  "sorted": lib.bbm_hip_set_sample_eval_sorted}[form]
            rc = fn(handle, flags, *frame, *s["out"], *some(s["xi"], xi), mask, count, 3, 0, *some(o[5:10], req),
                    *some(o[10:13], value), *some(o[13:16], weight), None)
        return rc, lib.bbm_hip_last_error()

    for what, kinds, args, text in REFUSED:
        for kind in kinds:
            a = {k: v for k, v in args.items() if kind == EVAL_PDF or k != "cos"}
            # lane order: the _tangent form always, the plain form where no tangent pointer is given
            forms = [("lanes", "tangent")] + ([("lanes", "plain")] if not any(a.get("tangent", NO3)) else [])
            got = {}
            for order, form in forms + [("plan", "sorted")]:
                rc, message = call(kind, order, form, **a)
                want = text
                if text is LENGTH:
                    asked = 0 if a["length"] is None else lengths[order] + a["length"]
                    want = LENGTH[order] % (asked, lengths[order])
                assert rc == L.ERR_INVALID_ARG and want in message, (what, kind, order, form, rc, message)
                got[form] = message
            if text is not LENGTH:
                assert len(set(got.values())) == 1, (what, kind, got)
    # a compact plan is refused in lane order ahead of everything else about the plan, the tangent's mixture alone first
    compact = c.mset.plan(c.ids, drop=True)
    for kind in BOTH:
        for form, args, text in (("plain", dict(flags=BAD_FLAGS, length=4), COMPACT), ("tangent", dict(length=4), COMPACT),
                                 ("tangent", dict(tangent=(True, True, False)), TANGENT)):
            rc, message = call(kind, "lanes", form, plan=compact._handle, **args)
            assert rc == L.ERR_INVALID_ARG and text in message, (kind, form, rc, message)
    compact.close()
    torch.cuda.synchronize()
    for order in lengths:
        assert bool((outs[order] == STAMP).all()), ("a refused call wrote an output", order)
    # and the call without a fault is taken, in every form: the lists above are refused for their faults alone
    for kind in BOTH:
        for order, form in (("lanes", "plain"), ("lanes", "tangent"), ("plan", "sorted")):
            assert call(kind, order, form)[0] == 0, (kind, order, form)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------ 2. lane order = gather, plan order, scatter

def check_orders(c, mset, plan, most):
    """most: every optional stream at once; else the fewest outputs the calls allow."""
    live = c.mask.bool()
    din, dout, xi, normal, tangent, mask = plan.gather(c.din, c.dout, c.xi, c.normal, c.tangent, mask=c.mask)
    # eval_pdf
    kw = dict(mode=3 if most else 2, cosine=most)
    lane = mset.eval_pdf(c.din, c.dout, mask=c.mask, plan=plan, normal=c.normal, tangent=c.tangent, **kw)
    slot = mset.eval_pdf(din, dout, mask=mask, plan=plan, order="plan", normal=normal, tangent=tangent, **kw)
    assert [t is None for t in lane] == [t is None for t in slot] == ([False] * 3 if most else [True, False])
    back = plan.scatter(*[t for t in slot if t is not None])
    got, want = bits(*lane), bits(*(back if isinstance(back, tuple) else (back,)))
    assert got.shape == want.shape == (5 if most else 1, N)
    assert torch.equal(got[:, live], want[:, live]), ("eval_pdf", most)
    # sample_eval
    kw = dict(value=most, weight=most)
    smp, v, w = mset.sample_eval(c.dout, c.xi, mask=c.mask, plan=plan, normal=c.normal, tangent=c.tangent, **kw)
    ssmp, sv, sw = mset.sample_eval(dout, xi, mask=mask, plan=plan, order="plan", normal=normal, tangent=tangent, **kw)
    assert (v is None) == (sv is None) == (w is None) == (sw is None) == (not most)
    sorted_ = [ssmp.direction, ssmp.pdf, ssmp.flag] + ([sv, sw] if most else [])
    got, want = bits(smp.direction, smp.pdf, smp.flag, v, w), bits(*plan.scatter(*sorted_))
    assert got.shape == want.shape == (11 if most else 5, N)
    assert torch.equal(got[:, live], want[:, live]), ("sample_eval", most)
    return got


def test_lane_order_is_gather_plan_order_scatter(batch):
    c = batch
    # the most streams: normal, tangent (a row reads it: its gather is a launch of its own), mask and every output
    check_orders(c, c.mset, c.plan, True)
    # the fewest: one output, and a tangent that no row reads, which is neither gathered nor given scratch
    with_tangent = check_orders(c, c.isotropic, c.iso_plan, False)
    smp, _, _ = c.isotropic.sample_eval(c.dout, c.xi, mask=c.mask, plan=c.iso_plan, normal=c.normal, value=False,
                                        weight=False)
    live = c.mask.bool()
    assert torch.equal(with_tangent[:, live], bits(smp.direction, smp.pdf, smp.flag)[:, live]), "an unread tangent changed a lane"
