"""bbm_hip_sample_eval / bbm_hip_sample_eval_table at the C-ABI boundary and the Python methods' argument checks (CPU
only, ctypes, nothing launched): the two symbols are exported and bound, the ABI version and the registry are what they
were, and every bad call is refused with the existing error codes, in the order of every per-model call (the id, the
parameter count, NULL pointers), before anything is allocated or launched.  What needs a GPU is in
tests/test_gpu_sample_eval.py."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

N = 16
CT = [0.5, 0.5, 0.5, 0.1, 1.3]


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def _buf():
    """A host buffer that stands for a device array: no call here gets as far as a launch."""
    return ctypes.cast((ctypes.c_float * N)(), ctypes.c_void_p)


def _call(lib, mid, p, k, n, ins=True, req=True, value=(1, 1, 1), weight=(1, 1, 1)):
    """bbm_hip_sample_eval with the given groups of pointers set (a buffer) or NULL."""
    keep = []

    def ptr(on):
        if not on:
            return None
        keep.append(_buf())
        return keep[-1]
    args = [ptr(ins) for _ in range(5)] + [None, n, 3, 0] + [ptr(req) for _ in range(5)] + \
           [ptr(v) for v in value] + [ptr(w) for w in weight] + [None]
    return lib.bbm_hip_sample_eval(mid, p, k, *args)


def test_symbols_exported_and_bound(lib):
    from bbm_amd import _lib
    for s in ("bbm_hip_sample_eval", "bbm_hip_sample_eval_table"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # one argument per parameter of the declaration: 3 + 5 inputs + mask + n, component, unit + 5 + 3 + 3 + stream
    assert len(_lib.SIGNATURES["bbm_hip_sample_eval"][1]) == 24
    assert len(_lib.SIGNATURES["bbm_hip_sample_eval_table"][1]) == 24


def test_abi_version_and_registry_unchanged(lib):
    assert lib.bbm_hip_abi_version() == 12
    assert lib.bbm_hip_num_models() == 49


def test_error_codes_and_their_order(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    # 1. unknown id, whatever else is wrong
    assert _call(lib, 99, p, 5, N) == _lib.ERR_INVALID_MODEL
    assert b"unknown model" in lib.bbm_hip_last_error()
    assert _call(lib, 99, None, 4, N, ins=False, req=False, value=(1, 0, 0)) == _lib.ERR_INVALID_MODEL
    # 2. wrong nparams, before any pointer is looked at
    assert _call(lib, ct, p, 4, N, ins=False, req=False, value=(1, 0, 0)) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert _call(lib, ct, None, 5, N) == _lib.ERR_INVALID_ARG
    # 3. NULL inputs or required outputs with n > 0
    assert _call(lib, ct, p, 5, N, ins=False) == _lib.ERR_INVALID_ARG
    assert b"NULL" in lib.bbm_hip_last_error()
    assert _call(lib, ct, p, 5, N, req=False) == _lib.ERR_INVALID_ARG
    assert b"sample output pointer is NULL" in lib.bbm_hip_last_error()
    # a half-given output group
    for group in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1)):
        assert _call(lib, ct, p, 5, N, value=group) == _lib.ERR_INVALID_ARG, group
        assert b"value output" in lib.bbm_hip_last_error()
        assert _call(lib, ct, p, 5, N, weight=group) == _lib.ERR_INVALID_ARG, group
        assert b"weight output" in lib.bbm_hip_last_error()
        assert _call(lib, ct, p, 5, N, value=(0, 0, 0), weight=group) == _lib.ERR_INVALID_ARG, group
    # the call-mode and runtime-aggregate bits are decoded as everywhere: the latter on fused aggregates only
    assert _call(lib, ct | _lib.RUNTIME_AGGREGATE, p, 5, N) == _lib.ERR_INVALID_MODEL
    assert _call(lib, ct | _lib.CALL_EXACT, p, 4, N) == _lib.ERR_INVALID_ARG


def test_n_zero_is_a_noop(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    assert _call(lib, ct, p, 5, 0, ins=False, req=False, value=(0, 0, 0), weight=(0, 0, 0)) == 0
    assert _call(lib, ct | _lib.CALL_EXACT, p, 5, 0, ins=False, req=False, value=(0, 0, 0), weight=(0, 0, 0)) == 0
    for name in ("He", "Merl", "Aggregate<Lambertian,Bagher>"):       # every row has the uniform call
        mid = lib.bbm_hip_model_id(name.encode())
        k = lib.bbm_hip_model_nparams(mid)
        q = (ctypes.c_float * max(k, 1))()
        assert _call(lib, mid, q, k, 0, ins=False, req=False, value=(0, 0, 0), weight=(0, 0, 0)) == 0, name


def test_table_call_on_null_table(lib):
    from bbm_amd import _lib
    for flags in (0, _lib.CALL_EXACT):
        for n in (0, N):
            assert lib.bbm_hip_sample_eval_table(None, flags, None, *([None] * 6), n, 3, 0,
                                                 *([None] * 12)) == _lib.ERR_INVALID_ARG
            assert b"table is NULL" in lib.bbm_hip_last_error()


def test_python_methods_exist():
    import bbm_amd
    assert hasattr(bbm_amd.BsdfModel, "sample_eval")
    assert hasattr(bbm_amd.MaterialTable, "sample_eval")
    assert hasattr(bbm_amd.AggregateModel, "sample_eval")
    assert "staged" in bbm_amd.AggregateModel.sample_eval.__doc__


def test_python_argument_errors_before_any_launch():
    import bbm_amd
    models = [bbm_amd.CookTorrance(), bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance())]
    out = torch.zeros((3, N), dtype=torch.float32)
    xi = torch.zeros((2, N), dtype=torch.float32)
    for m in models:
        with pytest.raises(TypeError):                  # doubleRGB is out of scope
            m.sample_eval(out.double(), xi.double())
        with pytest.raises(TypeError):
            m.sample_eval(out, xi.double())
        with pytest.raises(ValueError):                 # wrong shape
            m.sample_eval(out.t().contiguous(), xi)
        with pytest.raises(ValueError):
            m.sample_eval(torch.zeros((2, N), dtype=torch.float32), xi)
        with pytest.raises(TypeError):                  # wrong device type: host tensors
            m.sample_eval(out, xi)
