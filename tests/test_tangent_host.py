"""The tangent forms of the world-space calls at the C-ABI boundary and the Python argument checks (CPU only, ctypes,
nothing launched): the nine symbols are exported, declared and bound, the ABI version and the
registry are what they were, bbm_hip_model_anisotropic is 1 for exactly the nine rows whose parameters run along the
frame's X and Y, a partly NULL tangent is refused before anything else is looked at, n == 0 stays a no-op, and the
`tangent=` keyword follows its rules: without `normal=` and with `varying=` it is a ValueError, a bad tangent is
_normal_rows' TypeError or ValueError right after the normal's and ahead of every other argument.  What needs a GPU is
in tests/test_gpu_tangent.py."""
import ctypes
import functools
import inspect
import os
import re

import pytest

from tests import oracle_util as ou

torch = pytest.importorskip("torch")

N = 16
WARD = [0.5, 0.5, 0.5, 0.1, 0.4]
ANISOTROPIC = ["Ward", "WardDuer", "WardDuerGeislerMoroder", "CookTorranceHeitz", "GGXHeitz", "RibardiereAnisotropic",
               "Lafortune", "AshikhminShirley", "AshikhminShirleyFull"]
# symbol -> (its counterpart, where the tangent's three pointers stand in the argument list)
SYMBOLS = {
    "bbm_hip_frame_to_local_tangent": ("bbm_hip_frame_to_local", 3),
    "bbm_hip_frame_to_global_tangent": ("bbm_hip_frame_to_global", 3),
    "bbm_hip_sample_eval_world_tangent": ("bbm_hip_sample_eval_world", 6),
    "bbm_hip_sample_eval_table_world_tangent": ("bbm_hip_sample_eval_table_world", 6),
    "bbm_hip_eval_pdf_world_tangent": ("bbm_hip_eval_pdf_world", 6),
    "bbm_hip_eval_pdf_table_world_tangent": ("bbm_hip_eval_pdf_table_world", 6),
    "bbm_hip_set_eval_pdf_tangent": ("bbm_hip_set_eval_pdf", 5),
    "bbm_hip_set_sample_eval_tangent": ("bbm_hip_set_sample_eval", 5),
}


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def _buf():
    """A host buffer that stands for a device array: no call here gets as far as a launch."""
    return ctypes.cast((ctypes.c_float * N)(), ctypes.c_void_p)


def _ptrs(on, keep):
    out = []
    for o in on:
        keep.append(_buf() if o else None)
        out.append(keep[-1])
    return out


def test_symbols_exported_declared_and_bound(lib):
    from bbm_amd import _lib
    header = open(os.path.join(ou.ROOT, "include", "bbm_hip.h")).read()
    assert hasattr(lib, "bbm_hip_model_anisotropic") and "int bbm_hip_model_anisotropic(int model_id);" in header
    assert _lib.SIGNATURES["bbm_hip_model_anisotropic"] == (ctypes.c_int, [ctypes.c_int])
    for s, (base, at) in SYMBOLS.items():
        assert hasattr(lib, s), s
        assert f"int {s}(" in header, s
        res, args = _lib.SIGNATURES[s]
        bres, bargs = _lib.SIGNATURES[base]
        # the counterpart's signature with three pointers directly after nz
        assert res is bres and args == bargs[:at] + [ctypes.c_void_p] * 3 + bargs[at:], s
        decl = re.search(r"int %s\((.*?)\);" % s, header, re.S).group(1)
        names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
        assert names[at - 3:at + 3] == ["nx", "ny", "nz", "tx", "ty", "tz"], (s, names)
        bdecl = re.search(r"int %s\((.*?)\);" % base, header, re.S).group(1)
        bnames = [a.split()[-1].lstrip("*") for a in bdecl.split(",")]
        assert names[:at] + names[at + 3:] == bnames, s


def test_abi_version_and_registry_unchanged(lib):
    from tests.test_abi import REGISTRY_ORDER
    assert lib.bbm_hip_abi_version() == 12
    assert lib.bbm_hip_num_models() == 49
    assert [lib.bbm_hip_model_name(i).decode() for i in range(49)] == REGISTRY_ORDER


def test_model_anisotropic(lib):
    from bbm_amd import _lib
    import bbm_amd
    names = [lib.bbm_hip_model_name(i).decode() for i in range(49)]
    flags = [lib.bbm_hip_model_anisotropic(i) for i in range(49)]
    assert set(flags) == {0, 1}
    assert sorted(n for n, f in zip(names, flags) if f == 1) == sorted(ANISOTROPIC)
    assert sum(f == 0 for f in flags) == 40
    assert not any(f for n, f in zip(names, flags) if n.startswith("Aggregate<"))
    for bad in (-1, 49, 1000):
        assert lib.bbm_hip_model_anisotropic(bad) == _lib.ERR_INVALID_MODEL, bad
        assert b"unknown model id" in lib.bbm_hip_last_error()
    # the per-call mode bits are allowed in an id, as for the other attributes
    ward = lib.bbm_hip_model_id(b"Ward")
    assert lib.bbm_hip_model_anisotropic(ward | _lib.CALL_EXACT) == 1
    assert bbm_amd.Ward().anisotropic is True and bbm_amd.GGX().anisotropic is False
    assert bbm_amd.BsdfModel("Aggregate<Lambertian,NganWard>").anisotropic is False


PARTIAL = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]


def _call(lib, s, tangent, n=N, good=True, model=b"Ward"):
    """Symbol s with the given tangent pointers; good: every other pointer set (host buffers: a call that got as far
    as a launch would fault, none here does), else every other pointer NULL."""
    keep = []
    g = int(good)
    p = (ctypes.c_float * 5)(*WARD)
    mid = lib.bbm_hip_model_id(model)
    t = _ptrs(tangent, keep)
    three = lambda: _ptrs((g, g, g), keep)
    if s.startswith("bbm_hip_frame"):
        return getattr(lib, s)(*three(), *t, *three(), None, n, *three(), None)
    if "sample_eval" in s:
        body = three() + t + three() + _ptrs((g, g), keep) + [None, n, 3, 0] + _ptrs((g,) * 11, keep) + [None]
    else:
        body = three() + t + three() + three() + [None, n, 3, 0] + _ptrs((g,) * 5, keep) + [None]
    if "_table_" in s:
        return getattr(lib, s)(None, 0, None, *body)
    if "_set_" in s:
        return getattr(lib, s)(None, 0, *body)
    return getattr(lib, s)(mid, p, 5, *body)


def test_partly_null_tangent_is_refused_first(lib):
    from bbm_amd import _lib
    for s in SYMBOLS:
        for partial in PARTIAL:
            for good in (True, False):
                # ahead of every other check: the NULL table or plan, the other pointers
                assert _call(lib, s, partial, good=good) == _lib.ERR_INVALID_ARG, (s, partial)
                assert b"tangent: give tx, ty and tz or none" in lib.bbm_hip_last_error(), (s, partial)
            assert _call(lib, s, partial, n=0) == _lib.ERR_INVALID_ARG, (s, partial)
    # an isotropic row checks the tangent just the same
    for s in ("bbm_hip_sample_eval_world_tangent", "bbm_hip_eval_pdf_world_tangent"):
        assert _call(lib, s, (1, 0, 1), model=b"GGX") == _lib.ERR_INVALID_ARG


def test_other_checks_are_the_counterparts(lib):
    from bbm_amd import _lib
    for tangent in ((1, 1, 1), (0, 0, 0)):
        # the table and set calls reach the counterpart's first check; the uniform ones its pointer checks
        for s in SYMBOLS:
            if "_table_" in s:
                assert _call(lib, s, tangent) == _lib.ERR_INVALID_ARG and b"table is NULL" in lib.bbm_hip_last_error(), s
            elif "_set_" in s:
                assert _call(lib, s, tangent) == _lib.ERR_INVALID_ARG and b"plan is NULL" in lib.bbm_hip_last_error(), s
            else:
                assert _call(lib, s, tangent, good=False) == _lib.ERR_INVALID_ARG, s
                assert b"NULL" in lib.bbm_hip_last_error() and b"tangent" not in lib.bbm_hip_last_error(), s
    p = (ctypes.c_float * 5)(*WARD)
    ward = lib.bbm_hip_model_id(b"Ward")
    keep = []
    body = _ptrs((1,) * 12, keep) + [None, N, 3, 0] + _ptrs((1,) * 5, keep) + [None]
    assert lib.bbm_hip_eval_pdf_world_tangent(99, p, 5, *body) == _lib.ERR_INVALID_MODEL
    assert lib.bbm_hip_eval_pdf_world_tangent(ward, p, 4, *body) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()


def test_n_zero_is_a_noop(lib):
    from bbm_amd import _lib
    for tangent in ((1, 1, 1), (0, 0, 0)):
        for s in SYMBOLS:
            if "_table_" in s or "_set_" in s:
                continue        # a NULL handle is refused whatever n is, as by the counterparts
            assert _call(lib, s, tangent, n=0, good=False) == 0, s
            assert _call(lib, s, tangent, n=0, good=False, model=b"GGX") == 0, s
    # the id and the count are still checked
    p = (ctypes.c_float * 5)(*WARD)
    assert lib.bbm_hip_sample_eval_world_tangent(99, p, 5, *([None] * 12), 0, 3, 0, *([None] * 12)) == _lib.ERR_INVALID_MODEL


# ------------------------------------------------------------------------ the Python keyword

class _OnDevice(torch.Tensor):
    """A host tensor that says it is a CUDA tensor: it passes _normal_rows, so the checks behind the normal's can be
    reached on a machine without a GPU.  Nothing here reads it."""
    is_cuda = property(lambda self: True)


def _device_like(t):
    return t.as_subclass(_OnDevice)


def _callers():
    """(name, f(out-or-in, **kw)) for every method with tangent=, on a model, a tree, a table and a set; nothing here
    reaches a handle, so objects without one stand for the table and the set."""
    import bbm_amd
    ward = bbm_amd.Ward()
    tree = bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.Ward())

    class Table(bbm_amd.MaterialTable):
        def __init__(self):
            self._handle = None

    class Set(bbm_amd.MaterialSet):
        def __init__(self):
            self._handle = None

    t, s = Table(), Set()
    d = torch.zeros((3, N), dtype=torch.float32)
    xi = torch.zeros((2, N), dtype=torch.float32)
    fns = []
    for m, kw in ((ward, {}), (tree, {}), (t, dict(material=None)), (s, dict(material=None))):
        for name in ("eval_pdf", "eval", "pdf"):
            fns.append((f"{type(m).__name__}.{name}", functools.partial(getattr(m, name), d, d, **kw)))
        fns.append((f"{type(m).__name__}.sample_eval", functools.partial(m.sample_eval, d, xi, **kw)))
    fns.append(("to_local", lambda normal=None, **kw: bbm_amd.to_local(normal, d, **kw)))
    fns.append(("to_global", lambda normal=None, **kw: bbm_amd.to_global(normal, d, **kw)))
    return fns


def test_python_surface_exists():
    import bbm_amd
    for cls in (bbm_amd.BsdfModel, bbm_amd.MaterialTable, bbm_amd.MaterialSet, bbm_amd.AggregateModel):
        for name in ("eval_pdf", "sample_eval"):
            prm = inspect.signature(getattr(cls, name)).parameters["tangent"]
            assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
    for fn in (bbm_amd.to_local, bbm_amd.to_global):
        prm = inspect.signature(fn).parameters["tangent"]
        assert prm.default is None and prm.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert isinstance(bbm_amd.BsdfModel.anisotropic, property)


def test_python_keyword_rules_before_any_launch():
    import bbm_amd
    f32 = torch.zeros((3, N), dtype=torch.float32)
    normal = _device_like(f32)
    bad_tangents = [
        (f32.double(), TypeError),                                  # float64: floatRGB only
        (f32.numpy(), TypeError),                                   # not a tensor
        (torch.zeros((N, 3), dtype=torch.float32), ValueError),     # shape
        (torch.zeros((3, N + 1), dtype=torch.float32), ValueError),  # length
        (torch.zeros((3, 2 * N), dtype=torch.float32)[:, ::2], ValueError),     # stride
        (f32, TypeError),                                           # device: a host tensor
    ]
    for name, fn in _callers():
        with pytest.raises(ValueError, match="tangent= needs normal="):
            fn(tangent=_device_like(f32))
        with pytest.raises(ValueError, match="tangent= needs normal="):
            fn(tangent="not even a tensor")
        for tangent, exc in bad_tangents:
            with pytest.raises(exc, match="tangent"):
                fn(normal=normal, tangent=tangent)
        # the normal is checked first
        with pytest.raises(TypeError, match="normal"):
            fn(normal=f32, tangent=f32.double())
        # a good normal and tangent: the next check (the host directions, a table without a handle) refuses the call,
        # still before any launch
        with pytest.raises((TypeError, ValueError)) as e:
            fn(normal=normal, tangent=_device_like(f32))
        assert "tangent" not in str(e.value) and "normal" not in str(e.value), (name, e.value)
    # tangent= with varying= is refused as normal= is, whatever the tangent
    ward = bbm_amd.Ward()
    for fn in (ward.eval_pdf, ward.eval, ward.pdf):
        for tangent in (_device_like(f32), f32.double()):
            with pytest.raises(ValueError, match="to_local"):
                fn(f32, f32, normal=normal, tangent=tangent, varying={"roughness": torch.zeros((2, N))})
        with pytest.raises(ValueError, match="tangent= needs normal="):
            fn(f32, f32, tangent=_device_like(f32), varying={"roughness": torch.zeros((2, N))})
    # float64 directions: refused as with normal= alone
    for fn in (ward.eval_pdf, ward.eval, ward.pdf):
        with pytest.raises(TypeError, match="floatRGB only"):
            fn(f32.double(), f32.double(), normal=normal, tangent=_device_like(f32))
