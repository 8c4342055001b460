"""The image tools' host side (CPU only: no kernel runs): the PFM reader / writer against io/pfm.h's byte layout, the two
command lines' usage and error paths (bin/renderSphere.cpp:75-104, bin/plotBsdf.cpp:94-132), the count replay's
contract, and the new C-ABI entry points' argument checks, which all return before any launch."""
import ctypes
import importlib
import struct

import numpy as np
import pytest

from bbm_amd import _lib
from bbm_amd.pfm import export_pfm, import_pfm

render_mod = importlib.import_module("bbm_amd.render")
plot_mod = importlib.import_module("bbm_amd.plot")


# ------------------------------------------------------------------------------------------ PFM

def _image_3x2():
    # (3, H=2, W=3): channel c, row y, column x -> 100 c + 10 y + x
    c, y, x = np.meshgrid(np.arange(3), np.arange(2), np.arange(3), indexing="ij")
    return (100 * c + 10 * y + x).astype(np.float32)


def test_pfm_export_bytes(tmp_path):
    img = _image_3x2()
    f = tmp_path / "a.pfm"
    export_pfm(str(f), img)
    data = f.read_bytes()
    header = b"PF\n3 2\n-1.000000\n"
    assert data[:len(header)] == header
    # rows from y = height - 1 down to 0, pixels left to right, little-endian RGB triples
    want = []
    for y in (1, 0):
        for x in range(3):
            want += [img[0, y, x], img[1, y, x], img[2, y, x]]
    assert data[len(header):] == struct.pack("<18f", *want)


def test_pfm_channel_selection(tmp_path):
    img = _image_3x2()
    f = tmp_path / "c.pfm"
    export_pfm(str(f), img, channels=(2, -1, 7))
    back = import_pfm(str(f))
    np.testing.assert_array_equal(back[0], img[2])
    assert not back[1].any() and not back[2].any()


def test_pfm_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.standard_normal((3, 5, 7)).astype(np.float32)
    img[0, 0, 0], img[1, 2, 3] = np.float32(1e-42), np.float32(-0.0)       # a subnormal and a signed zero survive
    f = tmp_path / "r.pfm"
    export_pfm(str(f), img)
    back = import_pfm(str(f))
    assert back.dtype == np.float32 and back.shape == img.shape
    np.testing.assert_array_equal(back.view(np.uint32), img.view(np.uint32))


def test_pfm_import_big_endian_and_one_channel(tmp_path):
    img = _image_3x2()
    rows = img[:, ::-1].transpose(1, 2, 0)            # bottom-up (H, W, 3)
    big = tmp_path / "big.pfm"
    big.write_bytes(b"PF\n3 2\n1.000000\n" + rows.astype(">f4").tobytes())
    np.testing.assert_array_equal(import_pfm(str(big)), img)
    one = tmp_path / "one.pfm"
    one.write_bytes(b"Pf\n3 2\n-1.000000\n" + img[1, ::-1].astype("<f4").tobytes())
    got = import_pfm(str(one))
    np.testing.assert_array_equal(got[0], img[1])
    assert not got[1].any() and not got[2].any()
    bad = tmp_path / "bad.pfm"
    bad.write_bytes(b"XF\n1 1\n-1.000000\n" + bytes(12))
    with pytest.raises(RuntimeError):
        import_pfm(str(bad))


def test_pfm_empty_image_raises(tmp_path):
    with pytest.raises(RuntimeError):
        export_pfm(str(tmp_path / "e.pfm"), np.zeros((3, 0, 4), np.float32))
    with pytest.raises(RuntimeError):
        export_pfm(str(tmp_path / "e.pfm"), np.zeros((3, 4, 0), np.float32))


# ------------------------------------------------------------------------------------------ command lines

def test_render_cli_usage_and_errors(capsys, tmp_path):
    assert render_mod.main([]) == -1
    out = capsys.readouterr().out
    assert out.startswith("Usage:") and "[bsdfmodel=<bsdf string>] [filename=<name>] [light=[0,0,1]] [width=512] [height=512]" in out
    assert render_mod.main(["bsdfmodel=Lambertian()", "filename=x.pfm", "samples=3"]) == -1
    out = capsys.readouterr().out
    assert out.startswith("ERROR: invalid keywords:") and "samples" in out and out.rstrip().endswith(".")
    assert render_mod.main(["bsdfmodel=Lambertian()", "width=8"]) == -1
    assert capsys.readouterr().out == "ERROR: expected an output filename.\n"
    assert not list(tmp_path.iterdir())


def test_plot_cli_usage_and_errors(capsys):
    assert plot_mod.main([]) == -1
    out = capsys.readouterr().out
    assert out.startswith("Usage:") and "[maskZero] [plot=<eval|pdf|sample>]" in out and "[height=256]" in out
    assert plot_mod.main(["bsdfmodel=Lambertian()", "filename=x.pfm", "plot=eval", "light=[0,0,1]"]) == -1
    out = capsys.readouterr().out
    assert out.startswith("ERROR: invalid keywords:") and "light" in out
    assert plot_mod.main(["bsdfmodel=Lambertian()", "filename=x.pfm", "plot=brdf"]) == -1
    assert capsys.readouterr().out == "ERROR: unknown plotting command 'brdf'.\n"
    assert plot_mod.main(["bsdfmodel=Lambertian()", "filename=x.pfm"]) == -1        # no plot= at all
    assert capsys.readouterr().out == "ERROR: unknown plotting command ''.\n"
    assert plot_mod.main(["bsdfmodel=Lambertian()", "plot=pdf", "maskZero"]) == -1
    assert capsys.readouterr().out == "ERROR: expected an output filename.\n"


def test_names_exported():
    import bbm_amd
    assert bbm_amd.render_sphere is render_mod.render_sphere and bbm_amd.plot is plot_mod.plot
    assert "render_sphere" in bbm_amd.__all__ and "plot" in bbm_amd.__all__
    assert render_mod.parse_vec3("[1,-0.5,-1]") == [1.0, -0.5, -1.0] and render_mod.parse_vec3("0, 0, 1") == [0.0, 0.0, 1.0]


# ------------------------------------------------------------------------------------------ count replay

def replay(count, ndraws):
    """plotBsdf.cpp:80 after `count` hits of one bin: float += 1.0 / (float)(ndraws), the sum taken in double and
    rounded to float every time (backbone/array.h:87)."""
    a = 1.0 / float(np.float32(ndraws))
    v = np.float32(0)
    for _ in range(int(count)):
        v = np.float32(float(v) + a)
    return v


def test_count_replay_is_not_a_product():
    """Why the kernel replays the additions: the float after c additions is not float(c * addend) in general."""
    n = 2048
    vals = [replay(c, n) for c in (1, 3, 1000, 2048)]
    assert vals[0] == np.float32(1.0 / 2048) and vals[3] == np.float32(1.0)      # a power of two: every sum exact
    n = 333 * 7
    diff = sum(replay(c, n) != np.float32(c * (1.0 / float(np.float32(n)))) for c in range(0, 2331, 37))
    assert diff > 0


def replay_binades(count, ndraws):
    """The same float as replay(count, ndraws), a whole binade at a time -> (value, additions that moved it).

    While v = m u lies in [2^e, 2^(e+1)) (u = 2^(e-23), the float spacing) and v + a stays below 2^(e+1):
    double(v) + a rounds to the double grid d = 2^(e-52), and v is an even multiple of d, so the double sum is
    v + a_d with a_d = a rounded to d (ties to even in units of d: a's own parity); rounding v + a_d to float then
    adds q u when the rest r = a_d - q u is below u / 2 and (q + 1) u when it is above -- the same increment for every
    v of the binade.  r = u / 2 exactly is a tie, broken by m's parity: one addition at a time, as are the additions
    from 0 or a subnormal and the one that crosses into the next binade.  An addition that leaves the float where it
    was leaves it there for good (same v, same a)."""
    import math
    from fractions import Fraction
    a = 1.0 / float(np.float32(ndraws))
    exact_a = Fraction(a)
    v, left, moved = np.float32(0), int(count), 0
    while left > 0:
        bulk = 0
        if v >= np.finfo(np.float32).tiny:
            e = math.frexp(float(v))[1] - 1
            u, d, top = Fraction(2) ** (e - 23), Fraction(2) ** (e - 52), Fraction(2) ** (e + 1)
            a_d = round(exact_a / d) * d                      # Fraction.__round__: ties to even
            q, r = divmod(a_d, u)
            if 2 * r != u:
                inc = q * u if 2 * r < u else (q + 1) * u
                if inc == 0:
                    break
                bulk = min(left, max(0, math.ceil((top - exact_a - Fraction(float(v))) / inc)))
                if bulk:
                    v = np.float32(float(Fraction(float(v)) + bulk * inc))
        if bulk == 0:
            nv = np.float32(float(v) + a)
            if nv == v:
                break
            v, bulk = nv, 1
        left -= bulk
        moved += bulk
    return v, moved


@pytest.mark.parametrize("ndraws", [2331, 2048, 1000])
def test_replay_binades_equals_the_naive_loop(ndraws):
    """Every count 0 .. ndraws: the binade-stepping restatement gives the float of the one-addition-at-a-time loop.
    2331 = 7 x 3 x 111 (the addend is no power of two, every binade rounds), 2048 (every sum exact), 1000."""
    a = 1.0 / float(np.float32(ndraws))
    v, naive = np.float32(0), [np.float32(0)]
    for _ in range(ndraws):
        v = np.float32(float(v) + a)
        naive.append(v)
    rounded = 0
    for c in range(ndraws + 1):
        got, moved = replay_binades(c, ndraws)
        assert got.dtype == np.float32 and got.view(np.uint32) == naive[c].view(np.uint32), (c, got, naive[c])
        assert moved == c                                   # nothing stagnates this early
        rounded += int(naive[c] != np.float32(c * a))
    assert (rounded > 0) == (ndraws != 2048)


def test_replay_binades_stagnation_and_ties():
    """Draw counts beyond 2^24, count = every draw in one bin (a stand-alone C loop of v = (float)((double)v + a)
    gave the same three floats, and 18 073 720 moving additions for the first):
      41 943 040 = 2.5 x 2^24: in [0.5, 1) the addend is 0.4 float spacings -- the sum stops at 0.5;
      50 331 648 = 3 x 2^24: a third of a spacing there -- 0.5 as well;
      16 777 217: (float) rounds it to 2^24, the addend is 2^-24 and every sum up to 1.0 is exact; the last addition,
      1 + 2^-24, is a tie and rounds to the even 1.0."""
    v, moved = replay_binades(41943040, 41943040)
    assert v == np.float32(0.5) and moved == 18073720
    v, moved = replay_binades(50331648, 50331648)
    assert v == np.float32(0.5) and moved < 50331648
    v, moved = replay_binades(16777217, 16777217)
    assert v == np.float32(1.0) and moved == 1 << 24
    # short of the stagnation point the additions all count
    v, moved = replay_binades(1 << 20, 41943040)
    assert moved == 1 << 20 and v < np.float32(0.5)


# ------------------------------------------------------------------------------------------ C-ABI argument checks

@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _v3(*v):
    return (ctypes.c_float * 3)(*v)


def test_image_errors_before_launch(lib):
    p = (ctypes.c_float * 5)(0.5, 0.5, 0.5, 0.1, 1.3)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    img = ctypes.c_void_p(0x1000)          # never dereferenced: every call below fails before a launch
    light, view = _v3(0, 0, -1), _v3(0, 0, 1)
    nodirs = [None] * 7

    def render(mid=ct, npar=5, w=8, h=8, l=light, image=img):
        return lib.bbm_hip_render_sphere(mid, p, npar, w, h, l, image, *nodirs, None)

    def plot(mid=ct, npar=5, kind=0, w=8, h=4, v=view, samples=1, image=img, counts=None):
        return lib.bbm_hip_plot(mid, p, npar, kind, w, h, v, samples, 1.0, 0, None, None, 1, image, counts, None)

    assert render(mid=9999) == _lib.ERR_INVALID_MODEL and b"unknown model" in lib.bbm_hip_last_error()
    assert plot(mid=9999) == _lib.ERR_INVALID_MODEL
    assert render(npar=4) == _lib.ERR_INVALID_ARG and b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert plot(npar=4) == _lib.ERR_INVALID_ARG and b"expected 5 parameters" in lib.bbm_hip_last_error()
    for kw in (dict(w=0), dict(h=0)):
        assert render(**kw) == _lib.ERR_INVALID_ARG and b"width and height" in lib.bbm_hip_last_error()
        assert plot(**kw) == _lib.ERR_INVALID_ARG and b"width and height" in lib.bbm_hip_last_error()
    assert render(w=1 << 16, h=(1 << 15) + 1) == _lib.ERR_INVALID_ARG and b"2^31" in lib.bbm_hip_last_error()
    assert plot(w=1 << 16, h=(1 << 15) + 1) == _lib.ERR_INVALID_ARG and b"2^31" in lib.bbm_hip_last_error()
    assert render(image=None) == _lib.ERR_INVALID_ARG and b"image pointer is NULL" in lib.bbm_hip_last_error()
    assert plot(image=None) == _lib.ERR_INVALID_ARG and b"image pointer is NULL" in lib.bbm_hip_last_error()
    assert plot(kind=2, counts=None) == _lib.ERR_INVALID_ARG and b"counts pointer is NULL" in lib.bbm_hip_last_error()
    for bad in (_v3(0, 0, 0), _v3(float("nan"), 0, 1), _v3(float("inf"), 0, 1), None):
        assert render(l=bad) == _lib.ERR_INVALID_ARG and b"light must be" in lib.bbm_hip_last_error()
        assert plot(v=bad) == _lib.ERR_INVALID_ARG and b"view must be" in lib.bbm_hip_last_error()
    assert plot(samples=0) == _lib.ERR_INVALID_ARG and b"samples must be positive" in lib.bbm_hip_last_error()
    for kind in (-1, 3, 17):
        assert plot(kind=kind) == _lib.ERR_INVALID_ARG and b"unknown plot kind" in lib.bbm_hip_last_error()
    # the staged path's entry points
    d = [ctypes.c_void_p(0x1000)] * 7
    assert lib.bbm_hip_render_sphere_dirs(0, 4, light, *d, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_render_sphere_dirs(4, 4, _v3(0, 0, 0), *d, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_render_sphere_dirs(4, 4, light, *([None] * 7), None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_render_shade(0, *d[:6], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_render_shade(16, *d[:5], None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_dirs(4, 4, 0, None, None, 1, *d[:3], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_dirs(4, 4, 2, None, None, 1, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_dirs(4, 4, 2, d[0], None, 1, *d[:3], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_accumulate(2, 4, 4, 1, 1.0, None, None, 1, *d[:3], d[3], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_accumulate(0, 4, 4, 1, 1.0, None, None, 1, d[0], None, None, d[3], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_accumulate(1, 4, 4, 1, 1.0, None, None, 1, d[0], None, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_bin(4, 0, 8, *d[:4], 0, d[4], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_bin(4, 4, 8, *d[:4], 0, None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_counts_image(None, 4, 4, 1, 1.0, d[0], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_counts_image(d[0], 4, 4, 0, 1.0, d[1], None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_counts_image(d[0], 4, 4, 1, 1.0, None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_draws(1, 0, 16, None, None, None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_plot_draws(1, 0, 0, None, None, None) == 0        # n == 0 is a no-op


def test_sample_bin_edge_cap_on_the_reference():
    """tests/test_gpu_image.py sets aside draws whose continuous bin coordinate lies within 1e-4 of a bin edge (numpy's
    arctan2 need not be glibc's), at most 10 of its 2048: the reference's own samples at that test's models, views
    and uniforms stay within the cap."""
    from tests import oracle_util as ou
    if ou.ref() is None:
        pytest.skip("oracle/_ref not built")
    pytest.importorskip("torch")
    from tests import test_gpu_image as tg
    rng = np.random.default_rng(31)
    n = 2048
    u = (rng.integers(0, 1 << 24, size=(2, n)).astype(np.float32) / np.float32(1 << 24)).astype(np.float32)
    cases = {"Lambertian": [0.2, 0.5, 0.8], "CookTorrance": [0.3, 0.5, 0.7, 0.2, 1.5], "GGX": [0.7, 0.6, 0.5, 0.3, 1.4]}
    tree = ("Aggregate", [("Lambertian", np.float32([0.2, 0.3, 0.4])), ("CookTorrance", np.float32([0.6, 0.5, 0.4, 0.25, 1.6]))])
    rejected = 0
    for view in tg.VIEWS:
        v = np.repeat(np.asarray(tg.bbm_view(view), np.float32)[:, None], n, axis=1)
        res = [ou.ref_sample(k, np.float32(p), v, u)[0] for k, p in cases.items()] + [ou.ref_runtime_sample(tree, v, u)[0]]
        for r in res:
            bx, by = tg.bins_np(r[:3], 8, 4)
            assert (tg.near_edge(bx, 8) | tg.near_edge(by, 4)).sum() <= 10
        rejected += int((res[2][3] <= tg.EPS).sum())
    assert rejected > 0        # GGX: the views on which maskZero is tested do reject draws
