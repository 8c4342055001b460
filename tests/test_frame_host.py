"""The shading-frame calls at the C-ABI boundary and the Python argument checks (CPU only, ctypes, nothing launched):
bbm_hip_frame_to_local / _to_global and bbm_hip_sample_eval_world / _table_world are exported and bound, the ABI
version and the registry are what they were, every bad call is refused before anything is launched, and `normal=` is
checked ahead of every other argument: wrong dtype or device is a TypeError, wrong shape, length or stride a
ValueError.  What needs a GPU is in tests/test_gpu_frame.py."""
import ctypes
import os

import pytest

from tests import oracle_util as ou

torch = pytest.importorskip("torch")

N = 16
CT = [0.5, 0.5, 0.5, 0.1, 1.3]
SYMBOLS = ("bbm_hip_frame_to_local", "bbm_hip_frame_to_global", "bbm_hip_sample_eval_world",
           "bbm_hip_sample_eval_table_world")


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def _buf():
    """A host buffer that stands for a device array: no call here gets as far as a launch."""
    return ctypes.cast((ctypes.c_float * N)(), ctypes.c_void_p)


def _ptrs(on, count, keep):
    out = []
    for _ in range(count):
        keep.append(_buf() if on else None)
        out.append(keep[-1])
    return out


def _world(lib, mid, p, k, n, normal=True, ins=True, req=True, value=(1, 1, 1), weight=(1, 1, 1)):
    keep = []
    args = _ptrs(normal, 3, keep) + _ptrs(ins, 5, keep) + [None, n, 3, 0] + _ptrs(req, 5, keep) + \
        [_ptrs(v, 1, keep)[0] for v in value] + [_ptrs(w, 1, keep)[0] for w in weight] + [None]
    return lib.bbm_hip_sample_eval_world(mid, p, k, *args)


def _frame(fn, n, normal=True, ins=True, outs=True):
    keep = []
    return fn(*_ptrs(normal, 3, keep), *_ptrs(ins, 3, keep), None, n, *_ptrs(outs, 3, keep), None)


def test_symbols_exported_and_bound(lib):
    from bbm_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # one argument per parameter of the declaration
    assert len(_lib.SIGNATURES["bbm_hip_frame_to_local"][1]) == 12
    assert len(_lib.SIGNATURES["bbm_hip_frame_to_global"][1]) == 12
    assert len(_lib.SIGNATURES["bbm_hip_sample_eval_world"][1]) == 27
    assert len(_lib.SIGNATURES["bbm_hip_sample_eval_table_world"][1]) == 27
    header = open(os.path.join(ou.ROOT, "include", "bbm_hip.h")).read()
    for s in SYMBOLS:
        assert f"int {s}(" in header, s


def test_abi_version_and_registry_unchanged(lib):
    assert lib.bbm_hip_abi_version() == 12
    assert lib.bbm_hip_num_models() == 49


def test_frame_calls_null_pointers_and_n_zero(lib):
    from bbm_amd import _lib
    for fn in (lib.bbm_hip_frame_to_local, lib.bbm_hip_frame_to_global):
        for bad in ("normal", "ins", "outs"):
            assert _frame(fn, N, **{bad: False}) == _lib.ERR_INVALID_ARG, bad
            assert b"NULL" in lib.bbm_hip_last_error()
            assert _frame(fn, 0, **{bad: False}) == 0, bad          # n == 0 is a no-op, as for every batch call
        assert _frame(fn, 0) == 0


def test_world_call_error_codes_and_their_order(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    assert _world(lib, 99, p, 5, N) == _lib.ERR_INVALID_MODEL
    assert _world(lib, 99, None, 4, N, normal=False, ins=False, req=False) == _lib.ERR_INVALID_MODEL
    assert _world(lib, ct, p, 4, N, normal=False) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert _world(lib, ct, p, 5, N, normal=False) == _lib.ERR_INVALID_ARG
    assert b"normal direction pointer is NULL" in lib.bbm_hip_last_error()
    assert _world(lib, ct, p, 5, N, ins=False) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.bbm_hip_last_error()
    assert _world(lib, ct, p, 5, N, req=False) == _lib.ERR_INVALID_ARG
    assert b"sample output pointer is NULL" in lib.bbm_hip_last_error()
    for group in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1)):
        assert _world(lib, ct, p, 5, N, value=group) == _lib.ERR_INVALID_ARG, group
        assert b"value output" in lib.bbm_hip_last_error()
        assert _world(lib, ct, p, 5, N, weight=group) == _lib.ERR_INVALID_ARG, group
        assert b"weight output" in lib.bbm_hip_last_error()
    assert _world(lib, ct | _lib.RUNTIME_AGGREGATE, p, 5, N) == _lib.ERR_INVALID_MODEL
    assert _world(lib, ct | _lib.CALL_EXACT, p, 4, N) == _lib.ERR_INVALID_ARG


def test_world_call_n_zero_is_a_noop(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    none = dict(normal=False, ins=False, req=False, value=(0, 0, 0), weight=(0, 0, 0))
    assert _world(lib, ct, p, 5, 0, **none) == 0
    assert _world(lib, ct | _lib.CALL_EXACT, p, 5, 0, **none) == 0
    for name in ("He", "Merl", "Aggregate<Lambertian,Bagher>"):       # every row has the uniform call
        mid = lib.bbm_hip_model_id(name.encode())
        k = lib.bbm_hip_model_nparams(mid)
        q = (ctypes.c_float * max(k, 1))()
        assert _world(lib, mid, q, k, 0, **none) == 0, name


def test_table_world_call_on_null_table(lib):
    from bbm_amd import _lib
    for flags in (0, _lib.CALL_EXACT):
        for n in (0, N):
            assert lib.bbm_hip_sample_eval_table_world(None, flags, None, *([None] * 9), n, 3, 0,
                                                       *([None] * 12)) == _lib.ERR_INVALID_ARG
            assert b"table is NULL" in lib.bbm_hip_last_error()


def test_python_surface_exists():
    import inspect

    import bbm_amd
    assert callable(bbm_amd.to_local) and callable(bbm_amd.to_global)
    assert "to_local" in bbm_amd.__all__ and "to_global" in bbm_amd.__all__
    for cls in (bbm_amd.BsdfModel, bbm_amd.MaterialTable, bbm_amd.AggregateModel):
        sig = inspect.signature(cls.sample_eval)
        assert sig.parameters["normal"].default is None and \
            sig.parameters["normal"].kind is inspect.Parameter.KEYWORD_ONLY, cls
    assert "staged" in bbm_amd.AggregateModel.sample_eval.__doc__


def _bad_normals():
    """(normal, the exception it must raise), for N lanes; every one is refused before `out` is looked at."""
    f32 = torch.zeros((3, N), dtype=torch.float32)
    return [
        (f32.double(), TypeError),                                  # float64: floatRGB only
        (f32.half(), TypeError),
        (f32.numpy(), TypeError),                                   # not a tensor
        ((f32[0], f32[1], f32[2]), TypeError),
        (torch.zeros((N, 3), dtype=torch.float32), ValueError),     # shape
        (torch.zeros((3 * N,), dtype=torch.float32), ValueError),
        (torch.zeros((2, N), dtype=torch.float32), ValueError),
        (torch.zeros((3, N + 1), dtype=torch.float32), ValueError),  # length
        (torch.zeros((3, N - 1), dtype=torch.float32), ValueError),
        (torch.zeros((3, 2 * N), dtype=torch.float32)[:, ::2], ValueError),     # stride
        (torch.zeros((N, 3), dtype=torch.float32).t(), ValueError),
        (f32, TypeError),                                           # device: a host tensor
    ]


def test_python_normal_argument_errors_before_any_launch():
    import bbm_amd
    models = [bbm_amd.CookTorrance(), bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance())]
    out = torch.zeros((3, N), dtype=torch.float32)
    xi = torch.zeros((2, N), dtype=torch.float32)
    for normal, exc in _bad_normals():
        for m in models:
            with pytest.raises(exc):
                m.sample_eval(out, xi, normal=normal)
        with pytest.raises(exc):
            bbm_amd.MaterialTable.sample_eval(object(), out, xi, material=None, normal=normal)
        for fn in (bbm_amd.to_local, bbm_amd.to_global):
            with pytest.raises(exc):
                fn(normal, out)
    # normal=None stays today's path: the host tensors are refused by the checks of `out`
    for m in models:
        with pytest.raises(TypeError):
            m.sample_eval(out, xi, normal=None)
