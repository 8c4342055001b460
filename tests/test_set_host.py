"""Material sets at the C-ABI boundary and in the Python grouping (CPU only, ctypes, nothing launched): the new symbols
are bound, the argument errors that need no device are returned without one, and MaterialSet.from_models' grouping is
checked on the path that makes no table.  (The checks that need live handles are in tests/test_gpu_set.py.)"""
import ctypes

import numpy as np
import pytest

SYMBOLS = ["bbm_hip_set_create", "bbm_hip_set_destroy", "bbm_hip_set_size", "bbm_hip_set_rows", "bbm_hip_set_offset",
           "bbm_hip_set_plan_create", "bbm_hip_set_plan_destroy", "bbm_hip_set_plan_lanes", "bbm_hip_set_plan_capacity",
           "bbm_hip_set_plan_segments", "bbm_hip_set_plan_order", "bbm_hip_set_plan_geometry", "bbm_hip_set_eval_pdf",
           "bbm_hip_set_sample_eval"]


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from bbm_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # one argument per parameter of the declarations: the table calls' with (plan, call_flags) in place of
    # (table, call_flags, material), the normal always present, and the cosine
    assert len(_lib.SIGNATURES["bbm_hip_set_eval_pdf"][1]) == 21
    assert len(_lib.SIGNATURES["bbm_hip_set_sample_eval"][1]) == 26
    assert _lib.SIGNATURES["bbm_hip_set_eval_pdf"][1][12] is ctypes.c_size_t
    assert _lib.SIGNATURES["bbm_hip_set_sample_eval"][1][11] is ctypes.c_size_t


def test_abi_version_and_registry_unchanged(lib):
    assert lib.bbm_hip_abi_version() == 12
    assert lib.bbm_hip_num_models() == 49


def test_geometry(lib):
    tile, chunk = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.bbm_hip_set_plan_geometry(ctypes.byref(tile), ctypes.byref(chunk)) == 0
    assert tile.value >= 256 and tile.value % 256 == 0 and chunk.value >= 256
    assert lib.bbm_hip_set_plan_geometry(None, None) == 0


def test_create_errors_need_no_device(lib):
    from bbm_amd import _lib
    h = ctypes.c_void_p()
    some = (ctypes.c_void_p * 33)()          # 33 NULL tables
    assert lib.bbm_hip_set_create(None, 1, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert b"tables is NULL" in lib.bbm_hip_last_error() and h.value is None
    for count in (0, 33):
        assert lib.bbm_hip_set_create(some, count, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
        assert b"1 to 32 tables" in lib.bbm_hip_last_error() and h.value is None
    assert lib.bbm_hip_set_create(some, 2, None) == _lib.ERR_INVALID_ARG
    assert b"out is NULL" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_create(some, 2, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert b"table 0 is NULL" in lib.bbm_hip_last_error() and h.value is None


def test_handle_calls_on_null(lib):
    from bbm_amd import _lib
    assert lib.bbm_hip_set_destroy(None) == 0 and lib.bbm_hip_set_plan_destroy(None) == 0
    assert lib.bbm_hip_set_size(None) == 0 and lib.bbm_hip_set_rows(None) == 0
    assert lib.bbm_hip_set_plan_lanes(None) == 0 and lib.bbm_hip_set_plan_capacity(None) == 0
    assert lib.bbm_hip_set_plan_order(None) is None
    h = ctypes.c_void_p()
    assert lib.bbm_hip_set_plan_create(None, None, 0, None, ctypes.byref(h)) == _lib.ERR_INVALID_ARG
    assert b"set is NULL" in lib.bbm_hip_last_error() and h.value is None
    seg = (ctypes.c_uint64 * 4)()
    assert lib.bbm_hip_set_plan_segments(None, seg, 4) == _lib.ERR_INVALID_ARG
    for n in (0, 16):
        assert lib.bbm_hip_set_eval_pdf(None, 0, *([None] * 10), n, 3, 0, *([None] * 6)) == _lib.ERR_INVALID_ARG
        assert b"plan is NULL" in lib.bbm_hip_last_error()
        assert lib.bbm_hip_set_sample_eval(None, 0, *([None] * 9), n, 3, 0, *([None] * 12)) == _lib.ERR_INVALID_ARG
        assert b"plan is NULL" in lib.bbm_hip_last_error()


def test_grouping_makes_no_table():
    import bbm_amd
    from bbm_amd import _lib
    from bbm_amd.backbone import group_models
    assert {"MaterialSet", "MaterialPlan"} <= set(bbm_amd.__all__)
    lam = bbm_amd.Lambertian
    fused = lambda: bbm_amd.Aggregate(lam(), bbm_amd.CookTorrance())
    runtime = lambda: bbm_amd.Aggregate(lam(), bbm_amd.CookTorrance(), runtime=True)
    models = [bbm_amd.GGX(), "CookTorrance(eta = 1.5, roughness = 0.2)", fused(), bbm_amd.GGX(), runtime(), lam(),
              bbm_amd.CookTorrance(), fused(), runtime(), bbm_amd.GGX()]
    groups, ids = group_models(models)
    # order of first appearance; the runtime aggregate is a group of its own
    assert [(name, rt, len(ms)) for name, rt, ms in groups] == [
        ("GGX", False, 3), ("CookTorrance", False, 2), ("Aggregate<Lambertian,CookTorrance>", False, 2),
        ("Aggregate<Lambertian,CookTorrance>", True, 2), ("Lambertian", False, 1)]
    assert ids.dtype == np.int32
    assert ids.tolist() == [0, 3, 5, 1, 7, 9, 4, 6, 8, 2]
    # every model sits in its group at the place its id names
    flat = [m for _, _, ms in groups for m in ms]
    given = [bbm_amd.fromString(m) if isinstance(m, str) else m for m in models]
    for i, g in enumerate(ids):
        assert flat[g].name == given[i].name and flat[g].runtime == given[i].runtime
        assert (flat[g].parameter_values() == given[i].parameter_values()).all()
    assert flat[3] is not flat[0] and flat[1] is models[3]
    # refusals, by name
    with pytest.raises(_lib.BackboneError) as e:
        group_models([bbm_amd.GGX(), bbm_amd.BsdfModel("He")])
    assert e.value.code == _lib.ERR_UNSUPPORTED and "He: no material-table kernels" in str(e.value)
    with pytest.raises(_lib.BackboneError) as e:
        group_models([bbm_amd.BsdfModel("Aggregate<Lambertian,NganHe>")])
    assert "Aggregate<Lambertian,NganHe>" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        group_models([bbm_amd.GGX(), bbm_amd.AggregateModel(lam(), bbm_amd.CookTorrance())])
    assert "composed aggregates" in str(e.value)
    with pytest.raises(ValueError):
        group_models([])
    with pytest.raises(TypeError):
        group_models([bbm_amd.GGX(), 3])
    with pytest.raises(ValueError):
        bbm_amd.MaterialSet.from_models([])
    with pytest.raises(TypeError):
        bbm_amd.MaterialSet([bbm_amd.GGX()])
