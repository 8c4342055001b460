"""Material sets in plan order: compact plans (k_set_count<true>, k_set_place<true>), the public
permute (bbm_hip_set_plan_gather / _scatter over k_set_gather, k_set_gather_batched, k_set_scatter) and the calls on
streams that are already in slot order (bbm_hip_set_eval_pdf_sorted, bbm_hip_set_sample_eval_sorted), through
bbm_amd.MaterialPlan / MaterialSet and through ctypes.

"Bit for bit" = equal int32 views.  The contract: slot j with order()[j] = i returns what the lane-order set call
returns for lane i; a compact plan holds exactly the lanes whose id is in range.

  1. the compact plan against the partition worked out with numpy, and against a plain plan of the kept lanes;
  2. gather / scatter against numpy indexing on order();
  3. sorted == lane order, every output stream, plain and compact plans, aligned and shifted arrays;
  4. two bounces with no scatter in between;
  5. the C ABI with raw pointers, and the argument errors that need live handles.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
SEED = 0x50A7
ROWS = ["CookTorrance", "GGX", "Aggregate<Lambertian,CookTorrance>", "Ward"]     # Ward: the anisotropic row
SIZES = (3, 5, 4, 3)


def geometry():
    tile, chunk = ctypes.c_uint32(), ctypes.c_uint32()
    assert bbm_amd._lib.load().bbm_hip_set_plan_geometry(ctypes.byref(tile), ctypes.byref(chunk)) == 0
    return tile.value, chunk.value


def stream_limits():
    """kSetMaxIn and kSetMaxOut: the streams one gather and one scatter launch carry."""
    with open(os.path.join(ou.ROOT, "bbm_amd", "csrc", "set.hpp")) as f:
        src = f.read()
    return tuple(int(re.search(r"constexpr int " + k + r" = (\d+);", src).group(1)) for k in ("kSetMaxIn", "kSetMaxOut"))


def table_of(bbm, name, count):
    m = bbm.BsdfModel(name)
    scale = np.linspace(0.6, 1.0, count, dtype=F)[:, None]
    params = np.clip(m.parameter_values()[None] * scale, m.parameter_lower_bound(), m.parameter_upper_bound())
    return bbm.MaterialTable(name, params.astype(F))


def ids_t(ids):
    """Global ids (any integers; reduced mod 2^32) as the int32 CUDA tensor the calls take."""
    return torch.from_numpy((np.asarray(ids).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()


def partition(ids, offsets, drop):
    """The plan with numpy: (order with -1 in padding slots, segments).  Out of range: row 0, or (drop) no slot."""
    g = np.asarray(ids).astype(np.int64) & 0xFFFFFFFF
    off = np.asarray(offsets, np.int64)
    inside = g < off[-1]
    row = np.where(inside, np.searchsorted(off[1:-1], g, side="right"), -1 if drop else 0)
    order, seg = [], [0]
    for k in range(len(off) - 1):
        lanes = np.nonzero(row == k)[0]
        order += [lanes, np.full((-lanes.size) % 4, -1, np.int64)]
        seg.append(seg[-1] + lanes.size + (-lanes.size) % 4)
    return np.concatenate(order).astype(np.int64), seg


def id_patterns(n, offsets, rng):
    """Random, grouped, all one row, one row absent; a tenth out of range in each, 0xFFFFFFFF among them."""
    total, K = offsets[-1], len(offsets) - 1
    bad_values = np.array([-1, total, total + 7, 0x7FFFFFFF, -2**31])
    rnd = rng.integers(0, total, n)
    absent = rng.integers(offsets[1], total, n) if K > 1 else rnd            # row 0 absent
    one = rng.integers(offsets[K - 1], total, n)
    for how, ids in (("random", rnd), ("grouped", np.sort(rnd)), ("one row", one), ("row 0 absent", absent)):
        ids = ids.copy()
        bad = rng.random(n) < 0.1
        ids[bad] = bad_values[np.arange(int(bad.sum())) % bad_values.size]
        yield how, ids


def off1(x):
    """x's rows one element into a buffer of odd pitch: 4-byte aligned, not 16 (1-byte rows: not 4)."""
    buf = torch.zeros(x.shape[:-1] + (x.shape[-1] + 1,), dtype=x.dtype, device="cuda")
    buf[..., 1:] = x
    v = buf[..., 1:]
    assert v.data_ptr() % 16
    return v


def bits(*ts):
    """Tensors (1-D or (k, n)) as one (rows, n) int32 CUDA tensor of bit patterns."""
    return torch.cat([(t if t.dim() == 2 else t[None]).contiguous().view(torch.int32) for t in ts if t is not None])


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        diff = torch.nonzero((got != want).any(0))[:, 0]
        raise AssertionError((what, f"{diff.numel()} of {got.shape[1]} differ", diff[:8].tolist(),
                              got[:, diff[:2]].tolist(), want[:, diff[:2]].tolist()))


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


@pytest.fixture(scope="module")
def mset(bbm):
    return bbm.MaterialSet([table_of(bbm, name, m) for name, m in zip(ROWS, SIZES)])


@pytest.fixture(scope="module")
def scan_set(bbm):
    """32 one-material tables: the most rows, for the offset scan."""
    return bbm.MaterialSet([table_of(bbm, "Lambertian", 1) for _ in range(32)])


def lane_counts():
    tile, _ = geometry()
    return [1, 3, 4, 5, tile - 1, tile, tile + 1, 3 * tile + 5]


# ------------------------------------------------------------------------ 1. the compact plan

def check_plans(s, ids, what):
    n = len(ids)
    idt = ids_t(ids)
    for drop in (False, True):
        plan = s.plan(idt, drop=drop)
        order, seg = partition(ids, s.offsets, drop)
        assert plan.lanes == n and plan.compact is drop and plan.capacity == seg[-1], (what, drop)
        assert bbm_amd._lib.load().bbm_hip_set_plan_compact(plan._handle) == int(drop)
        assert plan.segments == seg, (what, drop, plan.segments, seg)
        got = plan.order().cpu().numpy().astype(np.int64)
        assert got.shape == order.shape and (got == order).all(), (what, drop, np.nonzero(got != order)[0][:8])
        if drop:
            g = np.asarray(ids).astype(np.int64) & 0xFFFFFFFF
            kept = np.nonzero(g < s.offsets[-1])[0]
            live = got[got >= 0]
            assert (np.sort(live) == kept).all(), (what, "exactly the lanes in range, each once")
            for k in range(s.rows):
                part = got[seg[k]:seg[k + 1]]
                part = part[part >= 0]
                assert (np.diff(part) > 0).all(), (what, k, "ascending within the segment")
            # the plain plan of the kept lanes alone has the same segments, and the same lanes renumbered
            removed = s.plan(ids_t(np.asarray(ids)[kept]))
            assert removed.segments == seg, (what, removed.segments, seg)
            ro = removed.order().cpu().numpy().astype(np.int64)
            assert (np.where(ro >= 0, kept[np.maximum(ro, 0)], -1) == got).all(), what
            removed.close()
        plan.close()


def test_compact_plan_is_the_partition_of_the_lanes_in_range(bbm, mset):
    rng = np.random.default_rng(SEED)
    for n in lane_counts():
        for how, ids in id_patterns(n, mset.offsets, rng):
            check_plans(mset, ids, (n, how))


def test_compact_plan_through_the_scan_loops_second_pass(bbm, scan_set):
    tile, chunk = geometry()
    groups = chunk // scan_set.rows + 1
    n = (groups - 1) * tile + 1                 # the smallest n whose rows x groups exceeds scan_chunk
    assert scan_set.rows * ((n + tile - 1) // tile) > chunk >= scan_set.rows * ((n - 1 + tile - 1) // tile)
    rng = np.random.default_rng(SEED + 1)
    how, ids = next(id_patterns(n, scan_set.offsets, rng))
    check_plans(scan_set, ids, (n, how))


def test_every_id_out_of_range(bbm, mset):
    n = geometry()[0] + 1
    ids = np.where(np.arange(n) % 2 == 0, -1, len(mset))
    plan = mset.plan(ids_t(ids), drop=True)
    assert plan.capacity == 0 and plan.segments == [0] * (mset.rows + 1) and plan.order().numel() == 0 and plan.lanes == n
    x = torch.rand((3, n), device="cuda")
    g, m = plan.gather(x, mask=True)
    assert g.shape == (3, 0) and m.shape == (0,)
    back = plan.scatter(g)
    assert back.shape == (3, n) and not bool(back.any())
    e3, e2 = torch.empty((3, 0), device="cuda"), torch.empty((2, 0), device="cuda")
    rgb, pdf, cos = mset.eval_pdf(e3, e3, plan=plan, order="plan", normal=e3, cosine=True)
    assert rgb.shape == (3, 0) and pdf.shape == (0,) and cos.shape == (0,)
    s, v, w = mset.sample_eval(e3, e2, plan=plan, order="plan")
    assert s.direction.shape == (3, 0) and s.flag.shape == (0,) and v.shape == (3, 0) and w.shape == (3, 0)
    with pytest.raises(ValueError, match="compact plan"):
        mset.eval_pdf(x, x, plan=plan)
    plan.close()


# ------------------------------------------------------------------------ 2. gather / scatter

def test_gather_and_scatter_against_numpy_indexing(bbm, mset):
    lib = bbm._lib.load()
    max_in, max_out = stream_limits()
    tile, _ = geometry()
    rng = np.random.default_rng(SEED + 2)
    dtypes = [(torch.float32, np.float32), (torch.int32, np.int32)]
    if hasattr(torch, "uint32"):
        dtypes.append((torch.uint32, np.uint32))
    for n in (5, tile + 1):
        how, ids = next(id_patterns(n, mset.offsets, rng))
        mask = rng.integers(0, 2, n).astype(np.uint8)
        for drop in (False, True):
            plan = mset.plan(ids_t(ids), drop=drop)
            order = plan.order().cpu().numpy().astype(np.int64)
            real = order >= 0
            assert drop or real.sum() == n
            for shape in (0, 1):
                assert lib.bbm_hip_set_gather_shape(shape) in (0, 1)
                for count in (1, max_in, max_out + 2):
                    for tdt, ndt in dtypes:
                        raw = rng.integers(0, 2**32, (count, n), dtype=np.uint64).astype(np.uint32)
                        raw[raw == 0] = 1                                   # a zero is what padding holds
                        x = torch.from_numpy(raw.view(ndt)).cuda()
                        assert x.dtype == tdt
                        want = np.where(real, raw[:, np.maximum(order, 0)], 0)
                        single = torch.from_numpy(raw[0].view(ndt)).cuda()
                        g, gm = plan.gather(x, mask=torch.from_numpy(mask).cuda())
                        g1 = plan.gather(single)
                        assert g.dtype == tdt and g.shape == (count, plan.capacity) and g1.shape == (plan.capacity,)
                        what = (n, drop, shape, count, str(tdt))
                        assert (g.cpu().numpy().view(np.uint32) == want).all(), what
                        assert (g1.cpu().numpy().view(np.uint32) == want[0]).all(), what
                        assert gm.dtype == torch.uint8 and (gm.cpu().numpy() == np.where(real, mask[np.maximum(order, 0)], 0)).all(), what
                        # scatter of a gather: the identity on the kept lanes, the sentinel elsewhere
                        sentinel = 0xDEADBEEF
                        out = torch.from_numpy(np.full((count, n), sentinel, np.uint32).view(ndt)).cuda()
                        back = plan.scatter(g, out=(out,))
                        assert back is out
                        kept = np.zeros(n, bool)
                        kept[order[real]] = True
                        assert (back.cpu().numpy().view(np.uint32) == np.where(kept, raw, sentinel)).all(), what
                        zeros = plan.scatter(g1)
                        assert (zeros.cpu().numpy().view(np.uint32) == np.where(kept, raw[0], 0)).all(), what
            lib.bbm_hip_set_gather_shape(0)
            # the mask rules: True is "every lane live"; a lone tensor comes back alone; no tensor, a mask alone
            live = plan.gather(mask=True)
            assert live.dtype == torch.uint8 and (live.cpu().numpy() == real.astype(np.uint8)).all()
            alone = plan.gather(torch.arange(n, dtype=torch.int32, device="cuda"))
            assert isinstance(alone, torch.Tensor) and (alone.cpu().numpy()[real] == order[real]).all()
            assert plan.gather() == ()
            # a slot-order tensor that is not 16-byte aligned is copied, not refused
            shifted = off1(alone)
            assert (plan.scatter(shifted).cpu().numpy()[kept] == np.arange(n)[kept]).all()
            with pytest.raises(ValueError):
                plan.gather(torch.zeros(n + 1, device="cuda"))
            with pytest.raises(TypeError):
                plan.gather(torch.zeros(n, dtype=torch.float64, device="cuda"))
            with pytest.raises(TypeError):
                plan.gather(torch.zeros(n))
            with pytest.raises(ValueError):
                plan.scatter(alone, out=(torch.zeros(n, device="cuda"),))       # another dtype
            plan.close()


# ------------------------------------------------------------------------ 3. sorted == lane order

class Common:
    pass


@pytest.fixture(scope="module")
def common(bbm, mset):
    from bbm_amd.plot import plot_draws
    c = Common()
    c.n = n = geometry()[0] + 1
    rng = np.random.default_rng(SEED + 3)
    c.din = bbm.fill_directions(SEED, 0, 0, n, mode=1)
    c.dout = bbm.fill_directions(SEED, 1, 0, n, mode=1)
    c.xi = plot_draws(SEED, 0, n)
    normal = rng.normal(size=(3, n)).astype(F) * rng.uniform(0.1, 3.0, n).astype(F)
    normal[:, 7::97] = 0                      # normals that are not live
    c.normal = torch.from_numpy(normal).cuda()
    tangent = rng.normal(size=(3, n)).astype(F)
    tangent[:, 5::89] = 0                     # tangents that fall back to the normal's frame
    c.tangent = torch.from_numpy(tangent).cuda()
    c.mask = torch.from_numpy(rng.integers(0, 2, n).astype(np.uint8)).cuda()
    how, c.ids = next(id_patterns(n, mset.offsets, rng))
    c.idt = ids_t(c.ids)
    c.plain = mset.plan(c.idt)
    c.compact = mset.plan(c.idt, drop=True)
    assert 0 < c.compact.capacity < c.plain.capacity
    c.lane_results = {}
    return c


FRAMES = [("local", False, False, False), ("world", True, False, False), ("world + cosine", True, False, True),
          ("tangent", True, True, False), ("tangent + cosine", True, True, True)]


def in_plan_order(c, plan, place):
    """The inputs through plan.gather, placed (aligned, or one element in)."""
    din, dout, xi, normal, tangent, mask = plan.gather(c.din, c.dout, c.xi, c.normal, c.tangent, mask=c.mask)
    order = plan.order().long()
    real = order >= 0
    return dict(din=place(din), dout=place(dout), xi=place(xi), normal=place(normal), tangent=place(tangent),
                mask=place(mask), lanes=order[real], real=real)


def frame_kw(x, world, tangent):
    return dict(normal=x["normal"] if world else None, tangent=x["tangent"] if tangent else None)


@pytest.mark.parametrize("kind", ["plain", "compact"])
@pytest.mark.parametrize("placed", ["aligned", "one element in"])
def test_eval_pdf_in_plan_order_bit_for_bit(bbm, mset, common, kind, placed):
    c = common
    plan = getattr(c, kind)
    place = off1 if placed == "one element in" else (lambda x: x)
    s = in_plan_order(c, plan, place)
    lane = dict(din=c.din, dout=c.dout, normal=c.normal, tangent=c.tangent)
    cap = plan.capacity
    for masked in (False, True):
        for what, world, tangent, cosine in FRAMES:
            for exact in (None, True, False):
                for mode in (1, 2, 3):
                    key = ("eval_pdf", masked, what, exact, mode)
                    if key not in c.lane_results:      # the lane-order call on the plain plan: once per combination
                        r = mset.eval_pdf(c.din, c.dout, mask=c.mask if masked else None, plan=c.plain, mode=mode,
                                          exact=exact, cosine=cosine, **frame_kw(lane, world, tangent))
                        c.lane_results[key] = bits(*r)
                    want = c.lane_results[key][:, s["lanes"]]
                    rgb = place(torch.empty((3, cap), device="cuda")) if mode & 1 else None
                    pdf = place(torch.empty((cap,), device="cuda")) if mode & 2 else None
                    r = mset.eval_pdf(tuple(s["din"]), tuple(s["dout"]), mask=s["mask"] if masked else None, plan=plan,
                                      order="plan", mode=mode, exact=exact, cosine=cosine, rgb=rgb, pdf=pdf,
                                      **frame_kw(s, world, tangent))
                    assert all(t is None or t.shape[-1] == cap for t in r)
                    same(bits(*r)[:, s["real"]], want, (kind, placed, key))
    # eval / pdf alone
    e = mset.eval(s["din"], s["dout"], plan=plan, order="plan", normal=s["normal"])
    p, cos = mset.pdf(s["din"], s["dout"], plan=plan, order="plan", normal=s["normal"], cosine=True)
    both = mset.eval_pdf(s["din"], s["dout"], plan=plan, order="plan", normal=s["normal"], cosine=True)
    same(bits(e, p, cos), bits(*both), (kind, placed, "eval, pdf"))


@pytest.mark.parametrize("kind", ["plain", "compact"])
@pytest.mark.parametrize("placed", ["aligned", "one element in"])
def test_sample_eval_in_plan_order_bit_for_bit(bbm, mset, common, kind, placed):
    c = common
    plan = getattr(c, kind)
    place = off1 if placed == "one element in" else (lambda x: x)
    s = in_plan_order(c, plan, place)
    lane = dict(normal=c.normal, tangent=c.tangent)

    def flat(res):
        smp, v, w = res
        return bits(smp.direction, smp.pdf, smp.flag, v, w)
    for masked in (False, True):
        for what, world, tangent, cosine in FRAMES:
            if cosine:
                continue
            for exact in (None, True, False):
                for value in (True, False):
                    for weight in (True, False):
                        key = ("sample_eval", masked, what, exact, value, weight)
                        if key not in c.lane_results:
                            c.lane_results[key] = flat(mset.sample_eval(
                                c.dout, c.xi, mask=c.mask if masked else None, plan=c.plain, exact=exact, value=value,
                                weight=weight, **frame_kw(lane, world, tangent)))
                        want = c.lane_results[key][:, s["lanes"]]
                        got = flat(mset.sample_eval(tuple(s["dout"]), tuple(s["xi"]), mask=s["mask"] if masked else None,
                                                    plan=plan, order="plan", exact=exact, value=value, weight=weight,
                                                    **frame_kw(s, world, tangent)))
                        assert got.shape[1] == plan.capacity
                        same(got[:, s["real"]], want, (kind, placed, key))


# ------------------------------------------------------------------------ 4. two bounces, no scatter

def test_two_bounces_without_a_scatter(bbm, mset, common):
    c = common
    n, total = c.n, len(mset)
    rng = np.random.default_rng(SEED + 4)
    pixel = torch.arange(n, dtype=torch.int32, device="cuda")
    light = bbm.fill_directions(SEED, 2, 0, n, mode=1)
    ids1 = rng.integers(0, total, n)
    # --- in plan order
    plan1 = mset.plan(ids_t(ids1))
    cap1 = plan1.capacity
    dout, xi, normal, light1, pixel1 = plan1.gather(c.dout, c.xi, c.normal, light, pixel)
    smp, _, w1 = mset.sample_eval(dout, xi, plan=plan1, order="plan", normal=normal, value=False)
    order1 = plan1.order().cpu().numpy().astype(np.int64)
    ids2 = rng.integers(0, total, cap1)                       # the next hits' materials, in slot order
    ids2[(order1 < 0) | (rng.random(cap1) < 0.2)] = -1        # padding, and the paths that ended
    plan2 = mset.plan(ids_t(ids2), drop=True)
    assert plan2.lanes == cap1 and 0 < plan2.capacity < cap1
    d2, normal2, light2, w2, pixel2 = plan2.gather(smp.direction, normal, light1, w1, pixel1)
    rgb, pdf, cos = mset.eval_pdf(light2, d2, plan=plan2, order="plan", normal=normal2, cosine=True)
    order2 = plan2.order().cpu().numpy().astype(np.int64)
    # --- in lane order, on plain plans
    plan_a = mset.plan(ids_t(ids1))
    smp_l, _, w_l = mset.sample_eval(c.dout, c.xi, plan=plan_a, normal=c.normal, value=False)
    ids2_l = np.full(n, -1, np.int64)
    ids2_l[order1[order1 >= 0]] = ids2[order1 >= 0]
    plan_b = mset.plan(ids_t(ids2_l))
    rgb_l, pdf_l, cos_l = mset.eval_pdf(light, smp_l.direction, plan=plan_b, normal=c.normal, cosine=True)
    # --- composed through the two orders: slot m of plan 2 is slot order2[m] of plan 1 is lane order1[order2[m]]
    real = order2 >= 0
    lanes = order1[order2[real]]
    kept = np.nonzero(ids2_l >= 0)[0]
    assert (lanes >= 0).all() and (np.sort(lanes) == kept).all(), "every surviving path exactly once"
    assert (pixel2.cpu().numpy()[real] == lanes).all(), "the pixel index names the lane"
    at = torch.from_numpy(lanes).cuda()
    realt = torch.from_numpy(real).cuda()
    same(bits(rgb, pdf, cos, w2, d2)[:, realt], bits(rgb_l, pdf_l, cos_l, w_l, smp_l.direction)[:, at], "two bounces")
    for p in (plan1, plan2, plan_a, plan_b):
        p.close()


# ------------------------------------------------------------------------ 5. the C ABI, and errors on live handles

def test_c_abi_with_raw_pointers(bbm, mset, common):
    c = common
    lib, L = bbm._lib.load(), bbm._lib
    E = L.ERR_INVALID_ARG
    plan = c.compact
    h, cap, n = plan._handle, plan.capacity, c.n
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = lambda t: [P(t[k]) for k in range(t.shape[0])]
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*[p.value for p in ps])
    # gather with raw pointers
    ins = [c.normal, c.din, c.dout, c.xi]
    sorted_ = [torch.empty((t.shape[0], cap), device="cuda") for t in ins]
    smask = torch.empty((cap,), dtype=torch.uint8, device="cuda")
    frm, to = arr([p for t in ins for p in rows(t)]), arr([p for t in sorted_ for p in rows(t)])
    assert lib.bbm_hip_set_plan_gather(h, frm, to, 11, P(c.mask), P(smask), n, None) == 0
    normal, din, dout, xi = sorted_
    want = plan.gather(*ins, mask=c.mask)
    same(bits(*sorted_, smask.int()), bits(*want[:4], want[4].int()), "raw gather")
    outs = torch.full((12, cap), 123.0, device="cuda")
    flag = torch.full((cap,), 77, dtype=torch.int32, device="cuda")
    R = rows(outs)
    no3 = [None, None, None]

    def ev(plan_=h, flags=0, nr=rows(normal), tan=no3, slots=cap, rgb=R[:3], pdf=R[3], cos=R[4]):
        return lib.bbm_hip_set_eval_pdf_sorted(plan_, flags, *nr, *tan, *rows(din), *rows(dout), P(smask), slots, 3, 0,
                                               *rgb, pdf, cos, None)

    def se(plan_=h, flags=0, nr=rows(normal), tan=no3, slots=cap, req=R[5:9], value=no3, weight=R[9:12], xi_=rows(xi)):
        return lib.bbm_hip_set_sample_eval_sorted(plan_, flags, *nr, *tan, *rows(dout), *xi_, P(smask), slots, 3, 0,
                                                  *req, P(flag), *value, *weight, None)
    refused = [
        (ev(slots=cap + 4), b"capacity"), (se(slots=cap - 4), b"capacity"), (ev(slots=n), b"capacity"),
        (se(slots=0), b"capacity"), (ev(plan_=None), b"plan is NULL"), (se(plan_=None), b"plan is NULL"),
        (ev(flags=L.CALL_EXACT | L.CALL_DEFAULT), b"call_flags"), (se(flags=1), b"call_flags"),
        (ev(nr=[P(normal[0]), None, P(normal[2])]), b"normal"), (se(nr=[None, P(normal[1]), None]), b"normal"),
        (ev(tan=[P(normal[0]), None, None]), b"tangent"), (se(tan=[None, None, P(normal[0])]), b"tangent"),
        (ev(nr=no3, tan=rows(normal), cos=None), b"tangent needs a normal"), (se(nr=no3, tan=rows(normal)), b"tangent needs a normal"),
        (ev(nr=no3), b"cos_in needs a normal"), (ev(rgb=no3, pdf=None, cos=None), b"every output pointer is NULL"),
        (ev(rgb=[R[0], None, R[2]]), b"eval output"), (se(req=[R[5], R[6], R[7], None]), b"sample output"),
        (se(value=[R[0], None, None]), b"value output"), (se(weight=[None, R[9], None]), b"weight output"),
        (se(xi_=[P(xi[0]), None]), b"xi pointer"),
    ]
    assert [rc for rc, _ in refused] == [E] * len(refused)
    for call, text in ((lambda: ev(slots=cap + 4), b"capacity"), (lambda: ev(nr=no3), b"cos_in needs a normal"),
                       (lambda: se(nr=no3, tan=rows(normal)), b"tangent needs a normal"),
                       (lambda: se(value=[R[0], None, None]), b"value output")):
        assert call() == E and text in lib.bbm_hip_last_error()
    # the permutes on a live plan
    one = arr([P(c.din[0])])
    dst = arr([P(din[0])])
    null = arr([ctypes.c_void_p(None)])
    off = arr([ctypes.c_void_p(din[0].data_ptr() + 4)])
    for rc, text in ((lib.bbm_hip_set_plan_gather(h, one, dst, 1, None, None, n - 1, None), b"plan was made for"),
                     (lib.bbm_hip_set_plan_scatter(h, dst, one, 1, cap, None), b"plan was made for"),
                     (lib.bbm_hip_set_plan_gather(h, null, dst, 1, None, None, n, None), b"NULL pointer"),
                     (lib.bbm_hip_set_plan_gather(h, one, null, 1, None, None, n, None), b"NULL pointer"),
                     (lib.bbm_hip_set_plan_scatter(h, null, one, 1, n, None), b"NULL pointer"),
                     (lib.bbm_hip_set_plan_gather(h, one, off, 1, None, None, n, None), b"16-byte aligned"),
                     (lib.bbm_hip_set_plan_scatter(h, off, one, 1, n, None), b"16-byte aligned"),
                     (lib.bbm_hip_set_plan_gather(h, one, dst, -1, None, None, n, None), b"count is negative"),
                     (lib.bbm_hip_set_plan_gather(h, one, dst, 1, P(c.mask), None, n, None), b"mask_from without mask_to"),
                     (lib.bbm_hip_set_plan_gather(h, None, None, 0, None, ctypes.c_void_p(smask.data_ptr() + 1), n, None),
                      b"4-byte aligned")):
        assert rc == E, text
    assert lib.bbm_hip_set_plan_gather(h, None, None, 0, None, None, n, None) == 0        # nothing to move
    assert lib.bbm_hip_set_plan_scatter(h, None, None, 0, n, None) == 0
    # the lane-order calls refuse a compact plan
    lane3 = lambda t: rows(t)
    for rc in (lib.bbm_hip_set_eval_pdf(h, 0, *lane3(c.normal), *lane3(c.din), *lane3(c.dout), None, n, 3, 0, *R[:3], R[3], None, None),
               lib.bbm_hip_set_eval_pdf_tangent(h, 0, *lane3(c.normal), *lane3(c.tangent), *lane3(c.din), *lane3(c.dout), None, n,
                                                3, 0, *R[:3], R[3], None, None),
               lib.bbm_hip_set_sample_eval(h, 0, *lane3(c.normal), *lane3(c.dout), *rows(c.xi), None, n, 3, 0, *R[5:9], P(flag),
                                           *no3, *R[9:12], None),
               lib.bbm_hip_set_sample_eval_tangent(h, 0, *lane3(c.normal), *lane3(c.tangent), *lane3(c.dout), *rows(c.xi), None,
                                                   n, 3, 0, *R[5:9], P(flag), *no3, *R[9:12], None)):
        assert rc == E and b"compact plan" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_plan_compact(h) == 1 and lib.bbm_hip_set_plan_compact(c.plain._handle) == 0
    assert lib.bbm_hip_set_plan_lanes(h) == n and lib.bbm_hip_set_plan_capacity(h) == cap
    torch.cuda.synchronize()
    assert bool((outs == 123.0).all()) and bool((flag == 77).all()), "a refused call wrote an output"
    # the empty plans: BBM_HIP_OK, nothing launched
    for create in (lib.bbm_hip_set_plan_create, lib.bbm_hip_set_plan_create_compact):
        he = ctypes.c_void_p()
        assert create(mset._handle, None, 0, None, ctypes.byref(he)) == 0 and he.value is not None
        assert lib.bbm_hip_set_plan_capacity(he) == 0
        assert lib.bbm_hip_set_eval_pdf_sorted(he, 0, *([None] * 13), 0, 3, 0, *([None] * 6)) == 0
        assert lib.bbm_hip_set_sample_eval_sorted(he, 0, *([None] * 12), 0, 3, 0, *([None] * 12)) == 0
        assert lib.bbm_hip_set_eval_pdf_sorted(he, 0, *([None] * 13), 4, 3, 0, *([None] * 6)) == E
        assert lib.bbm_hip_set_plan_gather(he, null, null, 1, None, None, 0, None) == 0
        assert lib.bbm_hip_set_plan_scatter(he, null, null, 1, 0, None) == 0
        assert lib.bbm_hip_set_plan_destroy(he) == 0
    hp = ctypes.c_void_p()
    assert lib.bbm_hip_set_plan_create_compact(mset._handle, None, n, None, ctypes.byref(hp)) == E and hp.value is None
    assert lib.bbm_hip_set_plan_create_compact(mset._handle, P(c.idt), n, None, None) == E
    assert lib.bbm_hip_set_plan_create_compact(mset._handle, P(c.idt), 0xFFFFFFF0, None, ctypes.byref(hp)) == E
    assert b"too large" in lib.bbm_hip_last_error() and hp.value is None
    # and the live calls, against the Python surface
    assert ev() == 0 and se() == 0
    rgb, pdf, cos = mset.eval_pdf(din, dout, mask=smask, plan=plan, order="plan", normal=normal, cosine=True)
    smp, _, w = mset.sample_eval(dout, xi, mask=smask, plan=plan, order="plan", normal=normal, value=False)
    same(bits(outs[:5], outs[5:9], flag, outs[9:12]), bits(rgb, pdf, cos, smp.direction, smp.pdf, smp.flag, w), "raw sorted calls")
