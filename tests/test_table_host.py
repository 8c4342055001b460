"""Material tables at the C-ABI boundary and in the Python constructor (CPU only, ctypes, nothing launched): which
rows have table kernels, and that create and the three batch calls refuse bad calls with the existing error codes
before anything is allocated or launched.  (The batch calls' checks that need a live table -- a NULL index or
direction pointer with n > 0 -- are in tests/test_gpu_table.py.)"""
import ctypes

import numpy as np
import pytest

UNSUPPORTED = ["He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"]


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def _create(lib, mid, p, k, m, out=True):
    h = ctypes.c_void_p()
    rc = lib.bbm_hip_table_create(mid, p, k, m, None, ctypes.byref(h) if out else None)
    assert h.value is None
    return rc


def test_supported_rows(lib):
    names = [lib.bbm_hip_model_name(i).decode() for i in range(lib.bbm_hip_num_models())]
    has = {name: lib.bbm_hip_model_has_table(i) for i, name in enumerate(names)}
    assert has == {name: lib.bbm_hip_model_has_varying(i) for i, name in enumerate(names)}
    assert has == {name: int(name not in UNSUPPORTED) for name in names}
    assert sum(has.values()) == 43 and len(names) == 49
    assert lib.bbm_hip_model_has_table(10_000) == -1
    assert b"10000" in lib.bbm_hip_last_error()


def test_python_introspection():
    import bbm_amd
    assert "MaterialTable" in bbm_amd.__all__
    assert bbm_amd.CookTorrance().has_table()
    assert bbm_amd.BsdfModel("Aggregate<Lambertian,Bagher>").has_table()
    assert not bbm_amd.BsdfModel("He").has_table()
    assert not bbm_amd.BsdfModel("Aggregate<Lambertian,NganHe>").has_table()
    assert not bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance()).has_table()


def test_create_errors_before_any_allocation(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 16)(*([0.5, 0.5, 0.5, 0.1, 1.3] * 3 + [0.0]))
    # unknown id first, then the unsupported row, whatever the other arguments are
    assert _create(lib, 99, p, 5, 1) == _lib.ERR_INVALID_MODEL
    assert b"unknown model" in lib.bbm_hip_last_error()
    assert _create(lib, 99, None, 0, 0, out=False) == _lib.ERR_INVALID_MODEL
    for name in UNSUPPORTED:
        mid = lib.bbm_hip_model_id(name.encode())
        k = lib.bbm_hip_model_nparams(mid)
        assert _create(lib, mid, p, k, 1) == _lib.ERR_UNSUPPORTED, name
        assert name.encode() in lib.bbm_hip_last_error()
        assert _create(lib, mid, None, k + 1, 0, out=False) == _lib.ERR_UNSUPPORTED, name
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    assert _create(lib, ct, p, 4, 3) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert _create(lib, ct, None, 5, 3) == _lib.ERR_INVALID_ARG
    assert b"params is NULL" in lib.bbm_hip_last_error()
    assert _create(lib, ct, p, 5, 0) == _lib.ERR_INVALID_ARG
    assert b"at least one material" in lib.bbm_hip_last_error()
    assert _create(lib, ct, p, 5, 3, out=False) == _lib.ERR_INVALID_ARG
    assert b"out is NULL" in lib.bbm_hip_last_error()
    # the call-mode bits belong to the batch calls' call_flags
    for bit in (_lib.CALL_EXACT, _lib.CALL_DEFAULT):
        assert _create(lib, ct | bit, p, 5, 3) == _lib.ERR_INVALID_ARG
        assert b"call_flags" in lib.bbm_hip_last_error()
    # the runtime-aggregate bit applies to fused aggregates only
    assert _create(lib, ct | _lib.RUNTIME_AGGREGATE, p, 5, 3) == _lib.ERR_INVALID_MODEL


def test_handle_calls_on_null(lib):
    from bbm_amd import _lib
    assert lib.bbm_hip_table_destroy(None) == 0
    assert lib.bbm_hip_table_model(None) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_table_size(None) == 0
    calls = {
        "eval_pdf": lambda flags, n: lib.bbm_hip_eval_pdf_table(None, flags, None, *([None] * 7), n, 3, 0,
                                                                None, None, None, None, None),
        "sample": lambda flags, n: lib.bbm_hip_sample_table(None, flags, None, *([None] * 6), n, 3, 0,
                                                            None, None, None, None, None, None),
        "reflectance": lambda flags, n: lib.bbm_hip_reflectance_table(None, flags, None, *([None] * 4), n, 3, 0,
                                                                      None, None, None, None),
    }
    for name, f in calls.items():
        for n in (0, 16):
            assert f(0, n) == _lib.ERR_INVALID_ARG, name
            assert b"table is NULL" in lib.bbm_hip_last_error()
            assert f(_lib.CALL_EXACT, n) == _lib.ERR_INVALID_ARG, name


def test_python_constructor_errors():
    import bbm_amd
    from bbm_amd import _lib
    good = np.tile(np.float32([0.5, 0.5, 0.5, 0.1, 1.3]), (3, 1))
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable("NoSuchModel", good)
    with pytest.raises(TypeError):
        bbm_amd.MaterialTable(bbm_amd.CookTorrance(), good)
    with pytest.raises(TypeError):
        bbm_amd.MaterialTable("CookTorrance", good.astype(np.float64))      # doubleRGB is out of scope
    with pytest.raises(TypeError):
        bbm_amd.MaterialTable("CookTorrance", good.astype(np.int32))
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable("CookTorrance", good[:, :4])
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable("CookTorrance", good[0])
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable("CookTorrance", good[:0])
    for name in UNSUPPORTED:
        k = bbm_amd.BsdfModel(name).parameter_values().size if name != "Merl" else 2
        with pytest.raises(_lib.BackboneError) as e:
            bbm_amd.MaterialTable(name, np.zeros((2, k), np.float32))
        assert e.value.code == _lib.ERR_UNSUPPORTED, name
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable.from_models([])
    with pytest.raises(ValueError):
        bbm_amd.MaterialTable.from_models([bbm_amd.CookTorrance(), bbm_amd.GGX()])
    with pytest.raises(ValueError):       # the same row with and without the runtime aggregate's semantics
        bbm_amd.MaterialTable.from_models([bbm_amd.Aggregate(bbm_amd.Lambertian(), bbm_amd.CookTorrance()),
                                           bbm_amd.Aggregate(bbm_amd.Lambertian(), bbm_amd.CookTorrance(), runtime=True)])
    with pytest.raises(ValueError):       # strings go through fromString
        bbm_amd.MaterialTable.from_models(["CookTorrance(eta = 1.5, roughness = 0.2)", bbm_amd.GGX()])
    with pytest.raises(TypeError):
        bbm_amd.MaterialTable.from_models([bbm_amd.CookTorrance(), 3])
    for runtime in (False, True):
        with pytest.raises(NotImplementedError):
            bbm_amd.MaterialTable.from_models([bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance(),
                                                                      runtime=runtime)])
