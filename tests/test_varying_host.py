"""Per-lane model parameters at the C-ABI boundary (CPU only, ctypes, no kernel runs): which rows have per-lane
kernels, and that the three entry points refuse bad calls with the existing error codes before anything is launched."""
import ctypes

import pytest

UNSUPPORTED = ["He", "HeWestin", "HeHolzschuch", "NganHe", "Aggregate<Lambertian,NganHe>", "Merl"]


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def _calls(lib):
    """The three entry points as f(model_id, params, nparams, varying, n) with every other pointer NULL."""
    return {
        "eval_pdf": lambda mid, p, k, v, n: lib.bbm_hip_eval_pdf_varying(mid, p, k, v, *([None] * 7), n, 3, 0,
                                                                         None, None, None, None, None),
        "sample": lambda mid, p, k, v, n: lib.bbm_hip_sample_varying(mid, p, k, v, *([None] * 6), n, 3, 0,
                                                                     None, None, None, None, None, None),
        "reflectance": lambda mid, p, k, v, n: lib.bbm_hip_reflectance_varying(mid, p, k, v, *([None] * 4), n, 3, 0,
                                                                               None, None, None, None),
    }


def test_supported_rows(lib):
    names = [lib.bbm_hip_model_name(i).decode() for i in range(lib.bbm_hip_num_models())]
    has = {name: lib.bbm_hip_model_has_varying(i) for i, name in enumerate(names)}
    assert set(UNSUPPORTED) <= set(names)
    assert has == {name: int(name not in UNSUPPORTED) for name in names}
    assert sum(has.values()) == 43 and len(names) == 49
    assert lib.bbm_hip_model_has_varying(10_000) == -1
    assert b"10000" in lib.bbm_hip_last_error()


def test_python_introspection():
    import bbm_amd
    assert bbm_amd.CookTorrance().has_varying()
    assert bbm_amd.BsdfModel("Aggregate<Lambertian,Bagher>").has_varying()
    assert not bbm_amd.BsdfModel("He").has_varying()
    assert not bbm_amd.BsdfModel("Aggregate<Lambertian,NganHe>").has_varying()


@pytest.mark.parametrize("call", ["eval_pdf", "sample", "reflectance"])
def test_errors_before_launch(lib, call):
    from bbm_amd import _lib
    f = _calls(lib)[call]
    p = (ctypes.c_float * 8)(*[0.5, 0.5, 0.5, 0.1, 1.3, 0, 0, 0])
    rows = (ctypes.c_void_p * 8)()
    # a row without per-lane kernels is refused before anything is launched
    for name, k in (("Merl", 2), ("He", 8)):
        assert f(lib.bbm_hip_model_id(name.encode()), p, k, None, 0) == _lib.ERR_UNSUPPORTED, name
        assert name.encode() in lib.bbm_hip_last_error()
        assert f(lib.bbm_hip_model_id(name.encode()), p, k, rows, 0) == _lib.ERR_UNSUPPORTED, name
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    # wrong parameter count, and NULL directions with n > 0
    assert f(ct, p, 4, None, 0) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert f(ct, p, 5, None, 16) == _lib.ERR_INVALID_ARG
    assert f(ct, p, 5, rows, 16) == _lib.ERR_INVALID_ARG
    assert f(ct, None, 5, None, 0) == _lib.ERR_INVALID_ARG
    # unknown id
    assert f(99, p, 5, None, 0) == _lib.ERR_INVALID_MODEL
    assert b"unknown model" in lib.bbm_hip_last_error()
    # n == 0 is a no-op, with or without rows, and with the call-mode and runtime-aggregate bits
    assert f(ct, p, 5, None, 0) == 0
    assert f(ct, p, 5, rows, 0) == 0
    assert f(ct | _lib.CALL_EXACT, p, 5, rows, 0) == 0
    agg = lib.bbm_hip_model_id(b"Aggregate<Lambertian,CookTorrance>")
    assert f(agg | _lib.RUNTIME_AGGREGATE, p, 8, rows, 0) == 0
