"""Material sets (bbm_amd/csrc/set.hpp, set.hip: k_set_count, k_set_scan, k_set_place, k_set_gather, k_set_scatter
behind bbm_hip_set_* and bbm_amd.MaterialSet / MaterialPlan).

The contract: a set is an ordered list of tables addressed by one global id per lane; every output of lane i is, bit
for bit ("bit for bit" = equal int32 views), what the matching table call returns for that lane on the table that
owns its id, with the id's index in that table; an id out of range is table 0's masked-index lane.

  1. the plan is the stable partition of the lanes by table, padded to quads per table;
  2. eval_pdf (three modes; local, world, world with the cosine; masks; exact) and sample_eval (local and world; value
     and weight on and off) against the per-table MaterialTable calls on each table's lanes, put together with torch
     indexing; aligned and one element into every buffer;
  3. the published library (tests/golden/fits.json) in one call, against the reference;
  4. one plan shared by two calls, a second stream, lifetimes, n == 0;
  5. the argument errors on live handles.
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
N = 1027
SEED = 0x5E7
META = ou.golden_meta()["models"]
SIZES = (3, 1, 4, 2, 7)
ROWS = ["CookTorrance", "Bagher", "Lambertian", "Aggregate<Lambertian,GGX>", "EPD"]


@pytest.fixture(scope="module")
def bbm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.cuda.set_device(0)
    return bbm_amd


def geometry():
    tile, chunk = ctypes.c_uint32(), ctypes.c_uint32()
    assert bbm_amd._lib.load().bbm_hip_set_plan_geometry(ctypes.byref(tile), ctypes.byref(chunk)) == 0
    return tile.value, chunk.value


def sets_of(name):
    """The row's golden parameter sets (params0..), (M, nparams) float32."""
    g = ou.golden_model(name)
    return np.stack([g[f"params{k}"].astype(F) for k in range(len(META[name]["sets"]))])


def ramp(m):
    t = np.linspace(0.0, 1.0, m, dtype=F)
    return np.stack([0.2 + 0.6 * t, 0.8 - 0.5 * t, 0.3 + 0.3 * t, 0.05 + 0.55 * t, 1.3 + 0.4 * t], 1).astype(F)


def ids_t(ids):
    """Global ids (any integers; reduced mod 2^32) as the int32 CUDA tensor the calls take."""
    return torch.from_numpy((np.asarray(ids).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda()


def rows_of(ids, offsets):
    """(row, local) of each id on the host: out of range is row 0 with index -1."""
    g = np.asarray(ids).astype(np.int64) & 0xFFFFFFFF
    off = np.asarray(offsets, np.int64)
    row = np.searchsorted(off[1:-1], g, side="right")
    inside = g < off[-1]
    row = np.where(inside, row, 0)
    local = np.where(inside, g - off[row], -1)
    return row, local.astype(np.int64)


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
    if not torch.equal(got, want):
        diff = torch.nonzero((got != want).any(0))[:, 0]
        raise AssertionError((what, f"{diff.numel()} lanes differ", diff[:8].tolist(), got[:, diff[:2]].tolist(),
                              want[:, diff[:2]].tolist()))


# ------------------------------------------------------------------------ 1. the plan

_PLAN_SETS = {}


def plan_set(bbm, K):
    """K tables of SIZES materials each (one row several times: a set may hold that)."""
    if K not in _PLAN_SETS:
        tables = [bbm.MaterialTable("CookTorrance", ramp(m)) for m in SIZES[:K]]
        _PLAN_SETS[K] = bbm.MaterialSet(tables)
    return _PLAN_SETS[K]


def lane_counts(K):
    tile, chunk = geometry()
    ns = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 1]
    # K * workgroups == scan_chunk + 1: the scan loop's second pass holds one entry.  Once, at the largest K that
    # divides it (the fewest lanes).
    if K == max(k for k in (1, 2, 5) if (chunk + 1) % k == 0):
        ns.append(((chunk + 1) // K - 1) * tile + 1)
    return ns


def id_patterns(n, offsets, rng):
    total, K = offsets[-1], len(offsets) - 1
    lanes = np.arange(n)
    edges = np.array([v for k in range(K + 1) for v in (offsets[k] - 1, offsets[k])] + [-1, total])
    yield "random", rng.integers(0, total, n)
    yield "one row", offsets[K - 1] + lanes % (offsets[K] - offsets[K - 1])
    yield "i % total", lanes % total
    yield "descending", (total - 1 - lanes % total)
    yield "boundaries", edges[lanes % edges.size]
    yield "out of range", np.where(lanes % 3 == 0, -1, np.where(lanes % 3 == 1, total, lanes % total))


def check_plan(plan, ids, offsets, what):
    n, K = len(ids), len(offsets) - 1
    seg = plan.segments
    assert len(seg) == K + 1 and seg[0] == 0, (what, seg)
    assert all(s % 4 == 0 for s in seg) and all(a <= b for a, b in zip(seg, seg[1:])), (what, seg)
    order = plan.order()
    assert order.dtype == torch.int32 and order.is_cuda and order.numel() == seg[-1], what
    order = order.cpu().numpy()
    row, _ = rows_of(ids, offsets)
    for k in range(K):
        lanes = np.nonzero(row == k)[0]
        part = order[seg[k]:seg[k + 1]]
        assert part.size - lanes.size in (0, 1, 2, 3), (what, k, part.size, lanes.size)
        assert (part[:lanes.size] == lanes).all(), (what, k, "not the ascending lanes of the row")
        assert (part[lanes.size:] == -1).all(), (what, k, "padding")
    live = order[order >= 0]
    assert live.size == n and (np.sort(live) == np.arange(n)).all(), (what, "every lane exactly once")


@pytest.mark.parametrize("K", [1, 2, 5])
def test_plan_is_the_stable_partition(bbm, K):
    s = plan_set(bbm, K)
    assert s.rows == K and len(s) == sum(SIZES[:K]) and s.offsets == [int(v) for v in np.cumsum((0,) + SIZES[:K])]
    tile, chunk = geometry()
    counts = lane_counts(K)
    if len(counts) == 16:
        assert K * ((counts[-1] + tile - 1) // tile) == chunk + 1
    rng = np.random.default_rng(SEED + K)
    for n in counts:
        for how, ids in id_patterns(n, s.offsets, rng):
            plan = s.plan(ids_t(ids))
            assert plan.lanes == n
            check_plan(plan, ids, s.offsets, (K, n, how))
            plan.close()


# ------------------------------------------------------------------------ 2. bit for bit against the table calls

class Common:
    pass


@pytest.fixture(scope="module")
def common(bbm):
    from bbm_amd.plot import plot_draws
    c = Common()
    c.rng = np.random.default_rng(SEED)
    c.din = bbm.fill_directions(SEED, 0, 0, N, mode=1)
    c.dout = bbm.fill_directions(SEED, 1, 0, N, mode=1)
    c.xi = plot_draws(SEED, 0, N)
    normal = c.rng.normal(size=(3, N)).astype(F) * c.rng.uniform(0.1, 3.0, N).astype(F)
    normal[:, 7::97] = 0                      # normals that are not live
    c.normal = torch.from_numpy(normal).cuda()
    c.mask = torch.from_numpy(c.rng.integers(0, 2, N).astype(np.uint8)).cuda()
    c.tables = [bbm.MaterialTable(name, sets_of(name)) for name in ROWS]
    c.set = bbm.MaterialSet(c.tables)
    total = len(c.set)
    rnd = c.rng.integers(0, total, N)
    bad = c.rng.random(N) < 0.05
    rnd[bad] = c.rng.choice([-1, total, total + 5, 0x7FFFFFFF, -2**31], int(bad.sum()))
    c.ids = {"mod": np.arange(N) % total, "random": rnd}
    assert 20 < bad.sum() < 100
    return c


def per_table(c, ids, call):
    """The other side of the comparison: `call(table, lanes, material)` -> (rows, lanes) bits for every table on its
    own lanes (torch indexing), put together lane by lane."""
    row, local = rows_of(ids, c.set.offsets)
    want = None
    for k, t in enumerate(c.tables):
        lanes = torch.from_numpy(np.nonzero(row == k)[0]).cuda()
        if lanes.numel() == 0:
            continue
        got = call(t, lanes, ids_t(local[row == k]))
        if want is None:
            want = torch.zeros((got.shape[0], N), dtype=torch.int32, device="cuda")
        want[:, lanes] = got
    return want


def pick(x, lanes):
    return None if x is None else x[..., lanes].contiguous()


@pytest.mark.parametrize("how", ["mod", "random"])
@pytest.mark.parametrize("placed", ["aligned", "one element in"])
def test_eval_pdf_bit_for_bit(bbm, common, how, placed):
    c = common
    ids = c.ids[how]
    place = off1 if placed == "one element in" else (lambda x: x)
    din, dout, normal, idt = place(c.din), place(c.dout), place(c.normal), place(ids_t(ids))
    plan = c.set.plan(idt)
    for mask in (None, c.mask):
        pmask = None if mask is None else place(mask)
        for world, cosine in ((False, False), (True, False), (True, True)):
            for exact in (None, True):
                for mode in (1, 2, 3):
                    kw = dict(mode=mode, exact=exact)

                    def call(t, lanes, material):
                        r = t.eval_pdf(pick(c.din, lanes), pick(c.dout, lanes), mask=pick(mask, lanes), material=material,
                                       normal=pick(c.normal, lanes) if world else None, cosine=cosine, **kw)
                        return bits(*r)
                    want = per_table(c, ids, call)
                    got = c.set.eval_pdf(tuple(din), tuple(dout), mask=pmask, plan=plan,
                                         normal=normal if world else None, cosine=cosine, **kw)
                    same(bits(*got), want, (how, placed, mask is not None, world, cosine, exact, mode))
    # the one-shot form, and eval / pdf alone
    r = c.set.eval_pdf(c.din, c.dout, material=ids_t(ids))
    same(bits(*r), per_table(c, ids, lambda t, l, m: bits(*t.eval_pdf(pick(c.din, l), pick(c.dout, l), material=m))),
         (how, "material="))
    same(bits(c.set.eval(c.din, c.dout, plan=plan), c.set.pdf(c.din, c.dout, plan=plan)), bits(*r), (how, "eval, pdf"))
    plan.close()


@pytest.mark.parametrize("how", ["mod", "random"])
@pytest.mark.parametrize("placed", ["aligned", "one element in"])
def test_sample_eval_bit_for_bit(bbm, common, how, placed):
    c = common
    ids = c.ids[how]
    place = off1 if placed == "one element in" else (lambda x: x)
    dout, xi, normal, idt = place(c.dout), place(c.xi), place(c.normal), place(ids_t(ids))
    plan = c.set.plan(idt)

    def flat(res):
        s, v, w = res
        return bits(s.direction, s.pdf, s.flag, v, w)
    for mask in (None, c.mask):
        pmask = None if mask is None else place(mask)
        for world in (False, True):
            for value in (True, False):
                for weight in (True, False):
                    kw = dict(value=value, weight=weight)

                    def call(t, lanes, material):
                        return flat(t.sample_eval(pick(c.dout, lanes), pick(c.xi, lanes), mask=pick(mask, lanes),
                                                  material=material, normal=pick(c.normal, lanes) if world else None, **kw))
                    want = per_table(c, ids, call)
                    got = c.set.sample_eval(tuple(dout), tuple(xi), mask=pmask, plan=plan,
                                            normal=normal if world else None, **kw)
                    same(flat(got), want, (how, placed, mask is not None, world, value, weight))
    plan.close()


# ------------------------------------------------------------------------ 3. the published library in one call

def published_lines(per_family=3):
    """A few accepted lines of every fits family that has table kernels: [(family key, line, parameters)]."""
    with open(os.path.join(ou.ROOT, "tests", "golden", "fits.json")) as f:
        fits = json.load(f)
    lib = bbm_amd._lib.load()
    chosen, seen = [], {}
    for fname in sorted(fits):
        for _, s, key, p in fits[fname]:
            if p is None or lib.bbm_hip_model_has_table(lib.bbm_hip_model_id(key.encode())) != 1:
                continue                      # a line the reference rejects, or a family without table kernels
            if seen.get((fname, key), 0) < per_family:
                seen[(fname, key)] = seen.get((fname, key), 0) + 1
                chosen.append((key, s, np.asarray(p, F)))
    return chosen


def test_published_library_in_one_call(bbm):
    lines = published_lines()
    families = sorted({k for k, _, _ in lines})
    assert len(families) >= 8 and all(p is not None for _, _, p in lines), families
    s = bbm.MaterialSet.from_models([line for _, line, _ in lines])
    assert s.rows == len(families) and len(s) == len(lines) and s.material_ids.dtype == np.int32
    assert sorted(s.material_ids.tolist()) == list(range(len(lines)))
    inp = ou.golden_inputs()
    pin, pout = inp["pin"], inp["pout"]
    n = pin.shape[1]
    which = np.arange(n) % len(lines)                       # the materials interleaved lane by lane
    din, dout = torch.from_numpy(pin).cuda(), torch.from_numpy(pout).cuda()
    rgb, pdf = s.eval_pdf(din, dout, material=ids_t(s.material_ids[which]))
    got = torch.cat([rgb, pdf[None]]).cpu().numpy()
    # the fused kernels of the same materials, one uniform call each: the set must return their bits
    uniform = np.zeros_like(got)
    ref = np.zeros_like(got) if ou.ref() is not None else None
    for j, (key, line, p) in enumerate(lines):
        m = bbm.fromString(line)
        assert m.name == key and m.runtime and (m.parameter_values() == p).all()
        lanes = np.nonzero(which == j)[0]
        r, q = m.eval_pdf(din[:, lanes].contiguous(), dout[:, lanes].contiguous())
        uniform[:, lanes] = torch.cat([r, q[None]]).cpu().numpy()
        if ref is not None:
            ref[:, lanes] = ou.ref_runtime_eval_pdf(ou.runtime_fit_tree(key, p), pin[:, lanes], pout[:, lanes])
    assert (got.view(np.int32) == uniform.view(np.int32)).all()
    if ref is not None:
        bad = set(zip(*ou.parity_violations(got, ref)))
        known = set(zip(*ou.parity_violations(uniform, ref)))
        print(f"{len(lines)} materials of {len(families)} families over {n} lanes: {len(bad)} values outside the bar, "
              f"{len(known)} in the uniform calls")
        assert bad <= known, sorted(bad - known)[:8]
    s.close()


# ------------------------------------------------------------------------ 4. plan reuse, streams, lifetimes

def test_plan_reuse_streams_and_lifetimes(bbm, common):
    c = common
    ids = c.ids["random"]
    idt = ids_t(ids)

    def done(kw):
        """The results are read on the current stream: after the call's own stream has finished."""
        if kw.get("stream") is not None:
            kw["stream"].synchronize()

    def nee(**kw):
        r = c.set.eval_pdf(c.din, c.dout, normal=c.normal, cosine=True, **kw)
        done(kw)
        return bits(*r)

    def bounce(**kw):
        s, v, w = c.set.sample_eval(c.dout, c.xi, normal=c.normal, value=False, **kw)
        done(kw)
        return bits(s.direction, s.pdf, s.flag, w)
    want_nee, want_bounce = nee(material=idt), bounce(material=idt)
    plan = c.set.plan(idt)
    same(nee(plan=plan), want_nee, "shared plan: eval_pdf")
    same(bounce(plan=plan), want_bounce, "shared plan: sample_eval")
    same(nee(plan=plan), want_nee, "shared plan: eval_pdf again")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = nee(plan=plan, stream=side)
    side.synchronize()
    same(got, want_nee, "side stream")
    side_plan = c.set.plan(idt, stream=side)
    got = bounce(plan=side_plan, stream=side)
    side.synchronize()
    same(got, want_bounce, "plan and call on the side stream")
    side_plan.close()
    # another n, material= with plan=, neither
    with pytest.raises(bbm._lib.BackboneError) as e:
        c.set.eval_pdf(c.din[:, :100].contiguous(), c.dout[:, :100].contiguous(), plan=plan)
    assert e.value.code == bbm._lib.ERR_INVALID_ARG and "plan was made for" in str(e.value)
    with pytest.raises(ValueError):
        c.set.eval_pdf(c.din, c.dout, material=idt, plan=plan)
    with pytest.raises(ValueError):
        c.set.sample_eval(c.dout, c.xi)
    other = bbm.MaterialSet(c.tables[:2])
    with pytest.raises(ValueError):
        other.eval_pdf(c.din, c.dout, plan=plan)
    # closed handles
    plan.close()
    plan.close()
    with pytest.raises(ValueError):
        c.set.eval_pdf(c.din, c.dout, plan=plan)
    with pytest.raises(ValueError):
        plan.order()
    other_plan = other.plan(idt)
    other.close()
    with pytest.raises(ValueError):
        other.eval_pdf(c.din, c.dout, material=idt)
    with pytest.raises(ValueError):
        other.eval_pdf(c.din, c.dout, plan=other_plan)
    with pytest.raises(ValueError):
        other.plan(idt)
    other_plan.close()
    # n == 0
    e3, e2 = torch.empty((3, 0), device="cuda"), torch.empty((2, 0), device="cuda")
    none = torch.empty((0,), dtype=torch.int32, device="cuda")
    empty = c.set.plan(none)
    assert empty.lanes == 0 and empty.segments == [0] * (c.set.rows + 1) and empty.order().numel() == 0
    rgb, pdf, cos = c.set.eval_pdf(e3, e3, plan=empty, normal=e3, cosine=True)
    assert rgb.shape == (3, 0) and pdf.shape == (0,) and cos.shape == (0,)
    s, v, w = c.set.sample_eval(e3, e2, material=none)
    assert s.direction.shape == (3, 0) and s.flag.shape == (0,) and v.shape == (3, 0) and w.shape == (3, 0)
    empty.close()


# ------------------------------------------------------------------------ 5. argument errors on live handles

def test_argument_errors_on_live_handles(bbm, common):
    c = common
    lib, L = bbm._lib.load(), bbm._lib
    n = 64
    idt = ids_t(c.ids["mod"][:n])
    plan = c.set.plan(idt)
    h, hs = plan._handle, c.set._handle
    assert lib.bbm_hip_set_size(hs) == len(c.set) and lib.bbm_hip_set_rows(hs) == len(ROWS)
    assert lib.bbm_hip_set_offset(hs, len(ROWS)) == len(c.set) and lib.bbm_hip_set_offset(hs, len(ROWS) + 1) == 0xFFFFFFFF
    assert lib.bbm_hip_set_plan_lanes(h) == n and lib.bbm_hip_set_plan_capacity(h) == plan.segments[-1]
    seg = (ctypes.c_uint64 * 8)()
    assert lib.bbm_hip_set_plan_segments(h, seg, 8) == len(ROWS) + 1 and list(seg)[:len(ROWS) + 1] == plan.segments
    assert lib.bbm_hip_set_plan_segments(h, seg, len(ROWS)) == L.ERR_INVALID_ARG
    assert lib.bbm_hip_set_plan_segments(h, None, 8) == L.ERR_INVALID_ARG
    # outputs that must stay untouched
    mark = 123.0
    outs = torch.full((12, n), mark, device="cuda")
    flag = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    d = [P(c.din[k]) for k in range(3)]
    o = [P(c.dout[k]) for k in range(3)]
    nr = [P(c.normal[k]) for k in range(3)]
    xi = [P(c.xi[k]) for k in range(2)]
    R = [P(outs[k]) for k in range(12)]
    no3 = [None, None, None]

    def ev(plan_=h, flags=0, normal=no3, din=d, n_=n, rgb=R[:3], pdf=R[3], cos=None):
        return lib.bbm_hip_set_eval_pdf(plan_, flags, *normal, *din, *o, None, n_, 3, 0, *rgb, pdf, cos, None)

    def se(plan_=h, flags=0, normal=no3, n_=n, req=R[:4], value=no3, weight=no3, xi_=xi):
        return lib.bbm_hip_set_sample_eval(plan_, flags, *normal, *o, *xi_, None, n_, 3, 0, *req, P(flag), *value,
                                           *weight, None)
    cases = [
        (ev(plan_=None), b"plan is NULL"), (se(plan_=None), b"plan is NULL"),
        (ev(flags=L.CALL_EXACT | L.CALL_DEFAULT), b"call_flags"), (se(flags=1), b"call_flags"),
        (ev(n_=n - 1), b"plan was made for"), (se(n_=n + 1), b"plan was made for"), (ev(n_=0), b"plan was made for"),
        (ev(normal=[nr[0], None, nr[2]]), b"normal"), (se(normal=[None, nr[1], None]), b"normal"),
        (ev(cos=R[4]), b"cos_in needs a normal"),
        (ev(rgb=no3, pdf=None), b"every output pointer is NULL"), (ev(normal=nr, rgb=no3, pdf=None, cos=R[4]), b"output"),
        (ev(rgb=[R[0], None, R[2]]), b"eval output"), (ev(din=[d[0], None, d[2]]), b"direction"),
        (se(req=[R[0], R[1], R[2], None]), b"sample output"), (se(value=[R[5], None, None]), b"value output"),
        (se(weight=[None, R[9], None]), b"weight output"), (se(xi_=[xi[0], None]), b"xi pointer"),
    ]
    for k, (rc, text) in enumerate(cases):
        assert rc == L.ERR_INVALID_ARG, (k, rc)
    # the message of each, call by call (the list above ran them all; the last error is the last one's)
    assert ev(cos=R[4]) == L.ERR_INVALID_ARG and b"cos_in needs a normal" in lib.bbm_hip_last_error()
    assert ev(normal=[nr[0], None, nr[2]]) == L.ERR_INVALID_ARG and b"normal" in lib.bbm_hip_last_error()
    assert ev(n_=n - 1) == L.ERR_INVALID_ARG and b"plan was made for" in lib.bbm_hip_last_error()
    assert ev(rgb=no3, pdf=None) == L.ERR_INVALID_ARG and b"every output pointer is NULL" in lib.bbm_hip_last_error()
    assert se(value=[R[5], None, None]) == L.ERR_INVALID_ARG and b"value output" in lib.bbm_hip_last_error()
    assert ev(plan_=None) == L.ERR_INVALID_ARG and b"plan is NULL" in lib.bbm_hip_last_error()
    torch.cuda.synchronize()
    assert bool((outs == mark).all()) and bool((flag == 77).all()), "a refused call wrote an output"
    # plan create on a live set
    hp = ctypes.c_void_p()
    assert lib.bbm_hip_set_plan_create(hs, None, n, None, ctypes.byref(hp)) == L.ERR_INVALID_ARG and hp.value is None
    assert b"material" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_plan_create(hs, P(idt), n, None, None) == L.ERR_INVALID_ARG
    assert lib.bbm_hip_set_plan_create(hs, P(idt), 0xFFFFFFF0, None, ctypes.byref(hp)) == L.ERR_INVALID_ARG
    assert b"too large" in lib.bbm_hip_last_error() and hp.value is None
    # a NULL table among live ones
    arr = (ctypes.c_void_p * 3)(c.tables[0]._handle.value, None, c.tables[1]._handle.value)
    assert lib.bbm_hip_set_create(arr, 3, ctypes.byref(hp)) == L.ERR_INVALID_ARG and hp.value is None
    assert b"table 1 is NULL" in lib.bbm_hip_last_error()
    # and the live calls still work
    assert ev(normal=nr, cos=R[4]) == 0 and se(normal=nr, weight=R[9:12]) == 0
    torch.cuda.synchronize()
    assert not bool((outs[:5] == mark).all(1).any())
    # Python: index dtype / device -> TypeError, length -> ValueError
    with pytest.raises(TypeError):
        c.set.eval_pdf(c.din, c.dout, material=ids_t(c.ids["mod"]).long())
    with pytest.raises(TypeError):
        c.set.plan(ids_t(c.ids["mod"]).cpu())
    with pytest.raises(ValueError):
        c.set.eval_pdf(c.din, c.dout, material=idt)
    with pytest.raises(ValueError):
        c.set.eval_pdf(c.din, c.dout, plan=plan, cosine=True)
    with pytest.raises(TypeError):
        c.set.eval_pdf(c.din.double(), c.dout.double(), plan=plan)
    plan.close()
