"""Every registry row through the image kernels (bbm_amd/csrc/image.hpp), and the corners of the model-independent ones
(image.hip).

DESIGN.md and image.hpp promise that the fused image kernels call the batch entry points' device functions in the same
order, so an image is, bit for bit, what the staged pipeline over eval / pdf / sample gives (directions -> the model's
batch call -> shade / accumulate / bin).  The batch calls are held to the reference for every model by
tests/test_gpu_parity.py; the identity carries that to k_render_sphere, k_plot and k_plot_sample of all rows, in the
default mode and, where a row has one, in its exact instantiation (k_plot<.., true>, k_plot_sample<exact_sample_t<M>>).
Every assertion here is bit or integer equality; nothing has a tolerance.

  1. fused image == staged pipeline, every row of model_names(), both modes;
  2. the count replay (k_count_image): rounding at a draw count that is no power of two, stagnation, draw counts
     beyond 2^24 -- against the naive replay and its binade-stepping restatement (tests/test_image_host.py);
  3. the second trip of the per-draw kernels' grid-stride loops (2^24 + 32 draws);
  4. plot_bin at chosen directions: poles, the zero vector, the axes, the column and row clamps, signed zeros;
  5. image calls on a side stream.
"""
import numpy as np
import pytest

import bbm_amd
from tests import oracle_util as ou
from tests.test_gpu_image import EPS, F, VIEWS, bbm_view, bins_np, bits, near_edge, replay_np, uniforms
from tests.test_image_host import replay_binades

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = bbm_amd.model_names()
META = ou.golden_meta()["models"]
RENDER_SHAPES = [(13, 17), (70, 5), (1, 1)]                      # (width, height)
LIGHTS = [(1, -0.5, -1), (0, 0, 1)]
PLOT_SHAPES = [(37, 9, 2), (1, 1, 3)]                            # (width, height, samples)
SAMPLE_SHAPE = (8, 4, 37)                                        # 1184 draws: no power of two
# a histogram fine enough that the exact samplers' last-bit differences cross bin edges (32768 columns, 2^18 draws)
FINE_SHAPE = (32768, 1, 8)

# Rows with an exact instantiation (math.hpp model_has_exact / has_exact_sample): the leaf, alone or as the second
# child of Aggregate<Lambertian, leaf>.  eval / pdf: the Beckmann, Student-T and Low NDFs' microfacet models
# (microfacet.hpp kHasExact), LowSmooth (lobes.hpp) and Bagher (spectral.hpp); sample: the Beckmann and GGX samplers'
# twins (microfacet.hpp exact_sample).  test_exact_rows_are_the_listed_ones checks the lists on the batch calls.
EXACT_EVAL_LEAVES = {"CookTorrance", "LowCookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "NganCookTorrance",
                     "Ribardiere", "RibardiereAnisotropic", "LowMicrofacet", "LowMicrofacetFit", "LowSmooth", "Bagher"}
EXACT_SAMPLE_LEAVES = {"CookTorrance", "LowCookTorrance", "CookTorranceWalter", "CookTorranceHeitz", "NganCookTorrance",
                       "GGX", "GGXHeitz"}


def _leaf(name):
    return name[len("Aggregate<Lambertian,"):-1] if name.startswith("Aggregate<Lambertian,") else name


def _cases(leaves):
    out = []
    for name in NAMES:
        out.append(pytest.param(name, None, id=f"{name}-default"))
        if _leaf(name) in leaves:
            out.append(pytest.param(name, True, id=f"{name}-exact"))
    return out


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
    """name -> the models a row is run with: Merl over the synthetic table; the golden file's first and last parameter
    sets; the row's defaults where there is no golden data."""
    def make(name):
        if name == "Merl":
            return [merl]
        sets = [None]
        if name in META:
            g = ou.golden_model(name)
            last = len(META[name]["sets"]) - 1
            sets = [g["params0"]] + ([g[f"params{last}"]] if last > 0 else [])
        out = []
        for p in sets:
            m = bbm.BsdfModel(name)
            if p is not None:
                m.set_parameter_values(p)
            out.append(m)
        return out
    return {name: make(name) for name in NAMES}


def _lib():
    return bbm_amd._lib.load()


def _check(rc):
    bbm_amd._lib.check(rc)


def _sptr(stream=None):
    return (torch.cuda.current_stream() if stream is None else stream).cuda_stream


def i32(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(i32(a), i32(b))


def view_rows(view, n):
    """normalize(view) in float32 (as the tool and the library do), once per draw -> (3, n) CUDA tensor."""
    return torch.from_numpy(np.repeat(np.asarray(bbm_view(view), F)[:, None], n, axis=1)).cuda()


def _used_on(stream, *tensors):
    """Tensors made here on the current stream and handed to a launch on `stream`: keep the allocator from reusing
    their memory before that stream is done with them."""
    if stream is not None:
        for t in tensors:
            t.record_stream(stream)
    return tensors[0]


# staged pipelines, from the public pieces bbm_amd/render.py and bbm_amd/plot.py use for an AggregateModel

def staged_render(m, w, h, din, dout, mask, exact=None, stream=None):
    npix = w * h
    i2, o2 = din.reshape(3, npix), dout.reshape(3, npix)
    mk = mask.reshape(npix).contiguous().view(torch.uint8)
    rgb = m.eval(i2, o2, mask=mk, exact=exact, stream=stream)
    img = _used_on(stream, torch.empty((3, h, w), dtype=torch.float32, device="cuda"), mk)
    _check(_lib().bbm_hip_render_shade(npix, rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(), i2[2].data_ptr(),
                                       mk.data_ptr(), img.data_ptr(), _sptr(stream)))
    return img


def staged_plot(m, kind, w, h, view, s, xi, scale=1.0, exact=None, stream=None):
    from bbm_amd.plot import KINDS, plot_directions
    ld = plot_directions(w, h, s, xi=xi, stream=stream)
    vd = view_rows(view, w * h * s)
    img = _used_on(stream, torch.empty((3, h, w), dtype=torch.float32, device="cuda"), vd)
    if kind == "eval":
        val = m.eval(ld, vd, exact=exact, stream=stream)
        r, g, b = val[0].data_ptr(), val[1].data_ptr(), val[2].data_ptr()
    else:
        val = m.pdf(ld, vd, exact=exact, stream=stream)
        r, g, b = val.data_ptr(), None, None
    _check(_lib().bbm_hip_plot_accumulate(KINDS[kind], w, h, s, float(scale), xi[0].data_ptr(), xi[1].data_ptr(), 1,
                                          r, g, b, img.data_ptr(), _sptr(stream)))
    return img


def plot_bin(w, h, d, pdf, mask_zero, stream=None):
    """bbm_hip_plot_bin over (3, n) directions and (n,) pdfs -> (h, w) int64 counts."""
    counts = _used_on(stream, torch.empty((h, w), dtype=torch.int64, device="cuda"))
    _check(_lib().bbm_hip_plot_bin(w, h, d.shape[1], d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), pdf.data_ptr(),
                                   int(bool(mask_zero)), counts.data_ptr(), _sptr(stream)))
    return counts


def counts_image(counts, w, h, s, scale=1.0, stream=None):
    img = _used_on(stream, torch.empty((3, h, w), dtype=torch.float32, device="cuda"))
    _check(_lib().bbm_hip_plot_counts_image(counts.data_ptr(), w, h, s, float(scale), img.data_ptr(), _sptr(stream)))
    return img


def staged_sample(m, w, h, view, s, xi, mask_zero, scale=1.0, exact=None, stream=None):
    smp = m.sample(_used_on(stream, view_rows(view, w * h * s)), xi, exact=exact, stream=stream)
    counts = plot_bin(w, h, smp.direction, smp.pdf, mask_zero, stream)
    return counts_image(counts, w, h, s, scale, stream), counts


# ------------------------------------------------------------------------ 1. fused image == batch entry points

def test_all_rows_are_listed(bbm):
    assert len(NAMES) == 49 and len(set(NAMES)) == 49 and "Merl" in NAMES
    known = {_leaf(n) for n in NAMES}
    assert EXACT_EVAL_LEAVES <= known and EXACT_SAMPLE_LEAVES <= known


def test_exact_rows_are_the_listed_ones(bbm, instances):
    """A row outside the lists has no exact instantiation: its batch calls give the same bits in both modes.  (A
    listed row may agree on a small batch -- the eval modes differ on values below 1e-30 only.)  The listed samplers
    do differ: their twins take glibc's erff / logf / sinf / cosf."""
    n = 4099
    din = bbm.fill_directions(0xBB5EED, 0, 0, n, mode=0)
    dout = bbm.fill_directions(0xBB5EED, 1, 0, n, mode=1)
    xi, _ = uniforms(n, 3)
    for name in NAMES:
        m = instances[name][0]
        if _leaf(name) not in EXACT_EVAL_LEAVES:
            a, b = m.eval_pdf(din, dout, exact=False), m.eval_pdf(din, dout, exact=True)
            assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), name
        a, b = m.sample(dout, xi, exact=False), m.sample(dout, xi, exact=True)
        same = same_bits(a.direction, b.direction) and same_bits(a.pdf, b.pdf) and torch.equal(a.flag, b.flag)
        assert same == (_leaf(name) not in EXACT_SAMPLE_LEAVES), name


@pytest.mark.parametrize("name,exact", _cases(EXACT_EVAL_LEAVES))
def test_render_fused_equals_staged(bbm, instances, name, exact):
    shaded = 0
    for m in instances[name]:
        for w, h in RENDER_SHAPES:
            for light in LIGHTS:
                img, din, dout, mask = bbm.render_sphere(m, w, h, light, return_dirs=True, exact=exact)
                want = staged_render(m, w, h, din, dout, mask, exact)
                assert same_bits(img[:, mask], want[:, mask]), (name, (w, h), light)
                assert not i32(img)[:, ~mask].any(), "unshaded pixels must be exactly 0"
                # without the directions' outputs the kernel writes the same image
                assert same_bits(bbm.render_sphere(m, w, h, light, exact=exact), img)
                shaded += int(mask.sum())
    assert shaded > 0


@pytest.mark.parametrize("kind", ["eval", "pdf"])
@pytest.mark.parametrize("name,exact", _cases(EXACT_EVAL_LEAVES))
def test_plot_fused_equals_staged(bbm, instances, name, exact, kind):
    for m in instances[name]:
        for w, h, s in PLOT_SHAPES:
            xi, _ = uniforms(w * h * s, 23)
            for view in VIEWS:
                got = bbm.plot(m, kind, w, h, view, s, xi=xi, exact=exact)
                want = staged_plot(m, kind, w, h, view, s, xi, exact=exact)
                assert same_bits(got, want), (name, kind, (w, h, s), view)        # NaN patterns included
        w, h, s = PLOT_SHAPES[0]
        got = bbm.plot(m, kind, w, h, VIEWS[1], s, 2.5, xi=xi_for(w, h, s), exact=exact)
        assert same_bits(got, staged_plot(m, kind, w, h, VIEWS[1], s, xi_for(w, h, s), 2.5, exact=exact)), (name, "scale")


def xi_for(w, h, s, seed=23):
    return uniforms(w * h * s, seed)[0]


@pytest.mark.parametrize("name,exact", _cases(EXACT_SAMPLE_LEAVES))
def test_plot_sample_fused_equals_staged(bbm, instances, name, exact):
    w, h, s = SAMPLE_SHAPE
    xi, _ = uniforms(w * h * s, 31)
    for m in instances[name]:
        for view in VIEWS:
            for mask_zero in (False, True):
                img, counts = bbm.plot(m, "sample", w, h, view, s, maskZero=mask_zero, xi=xi, return_counts=True,
                                       exact=exact)
                want_img, want = staged_sample(m, w, h, view, s, xi, mask_zero, exact=exact)
                assert counts.dtype == torch.int64 and torch.equal(counts, want), (name, view, mask_zero)
                assert same_bits(img, want_img), (name, view, mask_zero)
                assert int(counts.sum()) <= w * h * s and (mask_zero or int(counts.sum()) == w * h * s)


def test_exact_sampler_twins_reach_the_histogram(bbm):
    """k_plot_sample<exact_sample_t<M>>: on a histogram of 32768 columns the six exact samplers' counts equal the staged
    counts over the exact batch samples -- and those differ from the default mode's counts, so a histogram kernel
    that fell back to the default sampler would not pass (for a model whose batch samples are the same in both modes
    there would be nothing to tell apart)."""
    from tests.test_gpu_parity import EXACT_SAMPLERS
    w, h, s = FINE_SHAPE
    xi, _ = uniforms(w * h * s, 43)
    told_apart = []
    for name in EXACT_SAMPLERS:
        assert name in EXACT_SAMPLE_LEAVES
        m = bbm.BsdfModel(name)
        for view in VIEWS:
            img, counts = bbm.plot(m, "sample", w, h, view, s, xi=xi, return_counts=True, exact=True)
            want_img, want = staged_sample(m, w, h, view, s, xi, False, exact=True)
            assert torch.equal(counts, want) and same_bits(img, want_img), (name, view)
            _, default = staged_sample(m, w, h, view, s, xi, False, exact=False)
            _, fused_default = bbm.plot(m, "sample", w, h, view, s, xi=xi, return_counts=True, exact=False)
            assert torch.equal(fused_default, default), (name, view)
            if not torch.equal(want, default):
                told_apart.append(name)
    print("exact histograms that differ from the default mode's:", sorted(set(told_apart)))
    assert told_apart


def test_per_call_mode_wins_over_the_switch(bbm):
    """The per-call flag on both sides while the process-wide switch says the opposite (as
    test_gpu_parity.test_headline_size_parity): the images are those of the switch set the same way and no flag.
    CookTorrance for render, eval and pdf; the fine histogram for each exact sampler, at least one of which must
    differ between the modes for the comparison to bite."""
    from tests.test_gpu_parity import EXACT_SAMPLERS
    m = bbm.CookTorrance(albedo=[0.3, 0.5, 0.7], roughness=0.2, eta=1.5)
    samplers = [bbm.BsdfModel(name) for name in EXACT_SAMPLERS]
    (rw, rh), light = RENDER_SHAPES[0], LIGHTS[0]
    pw, ph, ps = PLOT_SHAPES[0]
    fw, fh, fs = FINE_SHAPE
    pxi, fxi = xi_for(pw, ph, ps), xi_for(fw, fh, fs, 43)
    view = VIEWS[1]

    def images(exact):
        out = [bbm.render_sphere(m, rw, rh, light, exact=exact)]
        out += [bbm.plot(m, kind, pw, ph, view, ps, xi=pxi, exact=exact) for kind in ("eval", "pdf")]
        for sm in samplers:
            out += list(bbm.plot(sm, "sample", fw, fh, view, fs, xi=fxi, return_counts=True, exact=exact))
        return out

    def staged(exact):
        _, din, dout, mask = bbm.render_sphere(m, rw, rh, light, return_dirs=True, exact=exact)
        out = [staged_render(m, rw, rh, din, dout, mask, exact)]
        out += [staged_plot(m, kind, pw, ph, view, ps, pxi, exact=exact) for kind in ("eval", "pdf")]
        for sm in samplers:
            out += list(staged_sample(sm, fw, fh, view, fs, fxi, False, exact=exact))
        return out

    def same(a, b):
        return same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)

    prev = bbm.set_exact_subnormals(False)
    try:
        plain = {}
        for exact in (False, True):
            bbm.set_exact_subnormals(exact)
            plain[exact] = images(None)
        differ = [name for k, name in enumerate(EXACT_SAMPLERS) if not torch.equal(plain[False][4 + 2 * k], plain[True][4 + 2 * k])]
        print("histograms that differ between the modes:", differ)
        assert differ, "no sampler's histogram differs between the modes: the comparison below would prove nothing"
        for exact in (False, True):
            bbm.set_exact_subnormals(not exact)
            for k, (got, want, ref) in enumerate(zip(images(exact), staged(exact), plain[exact])):
                assert same(got, want), (exact, k)
                assert same(got, ref), (exact, k)
    finally:
        bbm.set_exact_subnormals(prev)


# ------------------------------------------------------------------------ 2. the count replay

def test_count_replay_rounding(bbm):
    """7 x 3 x 111 = 2331 draws: the addend 1 / 2331 is no power of two, so the additions round and the replay is not
    a product."""
    w, h, s = 7, 3, 111
    n = w * h * s
    c = np.array([0, 1, 2, 3, 1000, 2330, 2331] + list(range(5, 2331, 167)), np.int64)
    assert c.size == w * h
    counts = torch.from_numpy(c.reshape(h, w)).cuda()
    want = replay_np(c, n)
    product = (c * (1.0 / float(F(n)))).astype(F)
    assert (bits(want) != bits(product)).any(), "the case proves nothing if the replay equals the product"
    assert all(bits(want[i]) == bits(replay_binades(c[i], n)[0]) for i in range(c.size))
    for scale in (1.0, 2.5):
        img = counts_image(counts, w, h, s, scale).cpu().numpy()
        for ch in range(3):
            np.testing.assert_array_equal(bits(img[ch].reshape(-1)), bits((want * F(scale)).astype(F)))


@pytest.mark.parametrize("samples,c_value", [(41943040, 0.5), (50331648, 0.5), (16777217, 1.0)])
def test_count_replay_stagnation_and_large_draw_counts(bbm, samples, c_value):
    """A 1 x 1 image holding every draw: the early exit on stagnation (0.5, where the addend is below half a float
    spacing), and (float)(npix * samples) beyond 2^24 -- 16 777 217 rounds to 2^24 and the last addition is a tie to
    even.  Expected from the binade-stepping restatement (checked on the CPU against the naive loop); the values of a
    stand-alone C loop are the cross-check."""
    want, _ = replay_binades(samples, samples)
    assert want == F(c_value)
    counts = torch.tensor([[samples]], dtype=torch.int64, device="cuda")
    img = counts_image(counts, 1, 1, samples).cpu().numpy()
    np.testing.assert_array_equal(bits(img.reshape(3)), np.repeat(bits(want), 3))
    # a count short of the stagnation point is not cut short
    part = (1 << 20) + 1
    img = counts_image(torch.tensor([[part]], dtype=torch.int64, device="cuda"), 1, 1, samples, 2.5).cpu().numpy()
    np.testing.assert_array_equal(bits(img.reshape(3)), np.repeat(bits(replay_binades(part, samples)[0] * F(2.5)), 3))


# ------------------------------------------------------------------------ 3. the grid-stride loops' second trip

def test_per_draw_kernels_wrap(bbm):
    """8 x 4 x (2^19 + 1) = 2^24 + 32 draws, 32 more than the per-draw kernels' grid (2^16 blocks of 256): k_plot_draws,
    k_plot_sample, k_plot_bin and k_plot_light_dirs against pieces that fit the grid.  Everything stays on the GPU."""
    from bbm_amd.plot import plot_directions, plot_draws
    w, h, cap = 8, 4, 1 << 24
    s = (1 << 19) + 1
    n = w * h * s
    assert n == cap + 32
    xi = plot_draws(17, 0, n)
    head, tail = plot_draws(17, 0, cap), plot_draws(17, cap, n - cap)
    assert torch.equal(xi[:, :cap], head) and torch.equal(xi[:, cap:], tail)
    del head, tail
    m = bbm.Lambertian(albedo=[0.2, 0.5, 0.8])
    view = VIEWS[1]
    _, counts = bbm.plot(m, "sample", w, h, view, s, xi=xi, return_counts=True)
    assert int(counts.sum()) == n
    vd = view_rows(view, n)
    pieces = []
    for lo, hi in ((0, cap), (cap, n)):
        x = xi[:, lo:hi].contiguous()
        smp = m.sample(vd[:, lo:hi].contiguous(), x)
        pieces.append(plot_bin(w, h, smp.direction, smp.pdf, False))
        del smp, x
    assert int(pieces[0].sum()) == cap and int(pieces[1].sum()) == n - cap
    assert torch.equal(counts, pieces[0] + pieces[1])
    smp = m.sample(vd, xi)
    assert torch.equal(plot_bin(w, h, smp.direction, smp.pdf, False), counts)
    del smp, vd
    # light directions: per pixel the first 2^19 draws (2^24 in all: one trip) and the last one (32 draws)
    full = plot_directions(w, h, s, xi=xi).view(3, w * h, s)
    xp = xi.view(2, w * h, s)
    first = plot_directions(w, h, s - 1, xi=xp[:, :, :s - 1].reshape(2, -1).contiguous()).view(3, w * h, s - 1)
    last = plot_directions(w, h, 1, xi=xp[:, :, s - 1:].reshape(2, -1).contiguous()).view(3, w * h, 1)
    for row in range(3):
        assert torch.equal(i32(full[row, :, :s - 1]), i32(first[row])), row
        assert torch.equal(i32(full[row, :, s - 1:]), i32(last[row])), row


# ------------------------------------------------------------------------ 4. plot_bin at chosen directions

def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.sqrt((v * v).sum())).astype(F)


LIFT = 0.05          # the axes raised off the equator (an exact equator point sits on a row edge)
NUDGE = 1e-3         # and turned off a column edge, to either side
CHOSEN = {
    "north pole": F([0, 0, 1]),
    "south pole (row clamp)": F([0, 0, -1]),
    "zero vector (rejected sample)": F([0, 0, 0]),
    "+x": _unit([1, 0, LIFT]), "+y": _unit([0, 1, LIFT]), "-x": _unit([-1, 0, LIFT]), "-y": _unit([0, -1, LIFT]),
    "+y before the edge": _unit([NUDGE, 1, LIFT]), "+y past the edge": _unit([-NUDGE, 1, LIFT]),
    "-x before the edge": _unit([-1, NUDGE, LIFT]), "-x past the edge": _unit([-1, -NUDGE, LIFT]),
    "-y before the edge": _unit([-NUDGE, -1, LIFT]), "-y past the edge": _unit([NUDGE, -1, LIFT]),
    "below +x": _unit([1, 0, -LIFT]),
    "phi + 2 pi reaches the width (column clamp)": _unit([1, -1e-9, 0.3]),
    "-x, y = +0": _unit([-1, 0.0, 0.3]), "-x, y = -0": _unit([-1, -0.0, 0.3]),
}
BIN_SHAPES = [(8, 4), (7, 4)]      # at width 8 the y and -x axes sit on column edges; at width 7 inside columns


def test_plot_bin_at_chosen_directions(bbm):
    """One direction per call, pdf = 1, mask_zero = 0, against bins_np and the clamp.  A direction is used at the
    shapes where its continuous coordinates keep 1e-4 from every interior edge (so the last bit of atan2 / asin cannot
    decide), and each is used at least once: at 8 x 4 the y and -x axes (phi a multiple of pi / 2) are column
    edges and are binned at 7 x 4, with their neighbours to either side of the edge at 8 x 4."""
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    used = {k: 0 for k in CHOSEN}
    seen = set()
    for w, h in BIN_SHAPES:
        for key, d in CHOSEN.items():
            bx, by = bins_np(d.reshape(3, 1), w, h)
            if (near_edge(bx, w) | near_edge(by, h)).any():
                continue
            used[key] += 1
            idx = int(np.minimum(by, F(h - 1)).astype(np.int64)[0] * w + np.minimum(bx, F(w - 1)).astype(np.int64)[0])
            want = np.zeros(w * h, np.int64)
            want[idx] = 1
            got = plot_bin(w, h, torch.from_numpy(d.reshape(3, 1)).cuda(), one, False).cpu().numpy()
            np.testing.assert_array_equal(got.reshape(-1), want, err_msg=f"{key} at {w} x {h}: bx {bx} by {by}")
            seen.add((w, h, idx))
    assert all(used.values()), used
    assert used["-x, y = +0"] == used["-x, y = -0"] == 1 and used["+y"] == 1       # width 7 only
    # what the list is for: the first and last row, the last column through the clamp, both sides of the edges
    assert (8, 4, 0) in seen and (8, 4, 3 * 8) in seen and any(i % 8 == 7 for w, _, i in seen if w == 8)
    bx, by = bins_np(CHOSEN["phi + 2 pi reaches the width (column clamp)"].reshape(3, 1), 8, 4)
    assert bx[0] == F(8) and bins_np(CHOSEN["south pole (row clamp)"].reshape(3, 1), 8, 4)[1][0] == F(4)
    # the whole list in one call
    w, h = 8, 4
    keys = [k for k, d in CHOSEN.items() if not (near_edge(bins_np(d.reshape(3, 1), w, h)[0], w)
                                                 | near_edge(bins_np(d.reshape(3, 1), w, h)[1], h)).any()]
    d = np.stack([CHOSEN[k] for k in keys], axis=1)
    bx, by = bins_np(d, w, h)
    idx = np.minimum(by, F(h - 1)).astype(np.int64) * w + np.minimum(bx, F(w - 1)).astype(np.int64)
    got = plot_bin(w, h, torch.from_numpy(d).cuda(), torch.ones(len(keys), dtype=torch.float32, device="cuda"), False)
    np.testing.assert_array_equal(got.cpu().numpy().reshape(-1), np.bincount(idx, minlength=w * h))


def test_plot_bin_mask_zero(bbm):
    """mask_zero counts a draw only if pdf > eps: 0 and eps are dropped, the next float above eps is counted."""
    w, h = 8, 4
    d = torch.from_numpy(np.repeat(F([0, 0, 1])[:, None], 3, axis=1)).cuda()
    pdf = torch.from_numpy(np.array([0.0, EPS, np.nextafter(EPS, F(1))], F)).cuda()
    want = np.zeros(w * h, np.int64)
    want[0] = 1
    np.testing.assert_array_equal(plot_bin(w, h, d, pdf, True).cpu().numpy().reshape(-1), want)
    want[0] = 3
    np.testing.assert_array_equal(plot_bin(w, h, d, pdf, False).cpu().numpy().reshape(-1), want)
    for k in range(3):
        got = plot_bin(w, h, d[:, k:k + 1].contiguous(), pdf[k:k + 1].clone(), True)
        assert int(got.sum()) == (1 if k == 2 else 0)


# ------------------------------------------------------------------------ 5. streams

@pytest.mark.parametrize("name", ["HeWestin", "EPD", "CookTorrance"])
def test_side_stream(bbm, instances, name):
    """render, plot eval and plot sample on a side stream (the He family's scratch CDF and EPD's prepared table are set
    up on that stream by the image path itself): the default stream's images, bit for bit."""
    m = instances[name][0]
    (rw, rh), light = RENDER_SHAPES[0], LIGHTS[0]
    pw, ph, ps = PLOT_SHAPES[0]
    sw, sh, ss = SAMPLE_SHAPE
    pxi, sxi = xi_for(pw, ph, ps), xi_for(sw, sh, ss, 31)
    view = VIEWS[1]

    def run(stream):
        out = [bbm.render_sphere(m, rw, rh, light, stream=stream),
               bbm.plot(m, "eval", pw, ph, view, ps, xi=pxi, stream=stream)]
        out += list(bbm.plot(m, "sample", sw, sh, view, ss, xi=sxi, return_counts=True, stream=stream))
        if name == "CookTorrance":        # the staged form as well
            _, din, dout, mask = bbm.render_sphere(m, rw, rh, light, return_dirs=True, stream=stream)
            out.append(staged_render(m, rw, rh, din, dout, mask, stream=stream))
            out.append(staged_plot(m, "eval", pw, ph, view, ps, pxi, stream=stream))
            out += list(staged_sample(m, sw, sh, view, ss, sxi, False, stream=stream))
        return out

    want = run(None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = run(side)
    side.synchronize()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
    if name == "CookTorrance":
        assert same_bits(got[0], got[4]) and same_bits(got[1], got[5]) and same_bits(got[2], got[6])
        assert torch.equal(got[3], got[7])
