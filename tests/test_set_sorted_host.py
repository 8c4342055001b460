"""Material sets in plan order at the C-ABI boundary and in the Python keywords (CPU only, ctypes, nothing launched;
DESIGN.md 4.21): the new symbols are bound with the header's signatures, the argument errors that need no live handle
are returned without one, and MaterialSet's order= / drop= rules are checked on objects that own no device memory.

A set needs tables and a table uploads its parameters, so no live plan exists without a device: the errors on live
handles (another n, slots != capacity, NULL entries, alignment, the lane-order calls' refusal of a compact plan) and
BBM_HIP_OK on the empty plan are in tests/test_gpu_set_sorted.py."""
import ctypes
import inspect
import os
import re

import pytest

from tests import oracle_util as ou

SYMBOLS = ["bbm_hip_set_plan_create_compact", "bbm_hip_set_plan_compact", "bbm_hip_set_plan_gather",
           "bbm_hip_set_plan_scatter", "bbm_hip_set_gather_shape", "bbm_hip_set_eval_pdf_sorted",
           "bbm_hip_set_sample_eval_sorted"]


@pytest.fixture(scope="module")
def lib():
    from bbm_amd import _lib
    return _lib.load()


def header_parameters(name):
    """The parameter list of `name`'s declaration in include/bbm_hip.h, one string per parameter."""
    with open(os.path.join(ou.ROOT, "include", "bbm_hip.h")) as f:
        src = f.read()
    m = re.search(r"^int " + name + r"\s*\(([^;]*)\);", src, re.M)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def ctype_of(param):
    if "*" in param:
        return ctypes.c_void_p
    kind = param.rsplit(" ", 1)[0]
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32}[kind]


def test_symbols_exported_with_the_headers_signatures(lib):
    from bbm_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        restype, argtypes = _lib.SIGNATURES[s]
        assert restype is ctypes.c_int, s
        params = header_parameters(s)
        assert [ctype_of(p) for p in params] == list(argtypes), (s, params)
    # the sorted calls are the *_tangent set calls with `slots` in place of n
    for sorted_, lanes in (("bbm_hip_set_eval_pdf_sorted", "bbm_hip_set_eval_pdf_tangent"),
                           ("bbm_hip_set_sample_eval_sorted", "bbm_hip_set_sample_eval_tangent")):
        assert _lib.SIGNATURES[sorted_] == _lib.SIGNATURES[lanes]
        a, b = header_parameters(sorted_), header_parameters(lanes)
        assert [p.replace("size_t slots", "size_t n") for p in a] == b
    assert len(header_parameters("bbm_hip_set_eval_pdf_sorted")) == 24
    assert len(header_parameters("bbm_hip_set_sample_eval_sorted")) == 29
    assert lib.bbm_hip_abi_version() == 12


def test_null_handles(lib):
    from bbm_amd import _lib
    E = _lib.ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.bbm_hip_set_plan_create_compact(None, None, 0, None, ctypes.byref(h)) == E
    assert b"set is NULL" in lib.bbm_hip_last_error() and h.value is None
    assert lib.bbm_hip_set_plan_create_compact(None, None, 16, None, None) == E
    assert lib.bbm_hip_set_plan_compact(None) < 0 and b"plan is NULL" in lib.bbm_hip_last_error()
    for n in (0, 16):
        assert lib.bbm_hip_set_eval_pdf_sorted(None, 0, *([None] * 13), n, 3, 0, *([None] * 6)) == E
        assert b"plan is NULL" in lib.bbm_hip_last_error()
        assert lib.bbm_hip_set_sample_eval_sorted(None, 0, *([None] * 12), n, 3, 0, *([None] * 12)) == E
        assert b"plan is NULL" in lib.bbm_hip_last_error()
        assert lib.bbm_hip_set_plan_gather(None, None, None, 0, None, None, n, None) == E
        assert b"plan is NULL" in lib.bbm_hip_last_error()
        assert lib.bbm_hip_set_plan_scatter(None, None, None, 0, n, None) == E
        assert b"plan is NULL" in lib.bbm_hip_last_error()


def test_sorted_calls_look_at_the_tangent_first(lib):
    """As the *_tangent calls: a partial tangent is found before anything else, a NULL plan included."""
    from bbm_amd import _lib
    some = ctypes.c_void_p(64)          # never dereferenced: the call is refused
    frame = [None, None, None, some, None, some]
    assert lib.bbm_hip_set_eval_pdf_sorted(None, 0, *frame, *([None] * 7), 16, 3, 0, *([None] * 6)) == _lib.ERR_INVALID_ARG
    assert b"tangent: give tx, ty and tz or none" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_sample_eval_sorted(None, 0, *frame, *([None] * 6), 16, 3, 0, *([None] * 12)) == _lib.ERR_INVALID_ARG
    assert b"tangent: give tx, ty and tz or none" in lib.bbm_hip_last_error()


def test_permute_errors_that_need_no_plan(lib):
    from bbm_amd import _lib
    E = _lib.ERR_INVALID_ARG
    arr = (ctypes.c_void_p * 2)()
    some = ctypes.c_void_p(64)          # never dereferenced: every call here is refused
    assert lib.bbm_hip_set_plan_gather(None, arr, arr, -1, None, None, 0, None) == E
    assert b"count is negative" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_plan_scatter(None, arr, arr, -1, 0, None) == E
    assert b"count is negative" in lib.bbm_hip_last_error()
    for frm, to in ((None, arr), (arr, None), (None, None)):
        assert lib.bbm_hip_set_plan_gather(None, frm, to, 2, None, None, 0, None) == E
        assert b"from or to is NULL" in lib.bbm_hip_last_error()
        assert lib.bbm_hip_set_plan_scatter(None, frm, to, 2, 0, None) == E
        assert b"from or to is NULL" in lib.bbm_hip_last_error()
    assert lib.bbm_hip_set_plan_gather(None, arr, arr, 0, some, None, 0, None) == E
    assert b"mask_from without mask_to" in lib.bbm_hip_last_error()


def test_gather_shape_switch(lib):
    from bbm_amd import _lib
    assert lib.bbm_hip_set_gather_shape(0) == 0          # the default
    assert lib.bbm_hip_set_gather_shape(1) == 0 and lib.bbm_hip_set_gather_shape(0) == 1
    for bad in (-1, 2):
        assert lib.bbm_hip_set_gather_shape(bad) == _lib.ERR_INVALID_ARG
    assert lib.bbm_hip_set_gather_shape(0) == 0


# ------------------------------------------------------------------------ the Python keywords

def test_signatures():
    import bbm_amd
    sig = inspect.signature(bbm_amd.MaterialSet.plan)
    assert sig.parameters["drop"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["drop"].default is False
    sig = inspect.signature(bbm_amd.MaterialPlan.__init__)
    assert sig.parameters["drop"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["drop"].default is False
    for name in ("eval_pdf", "sample_eval"):
        p = inspect.signature(getattr(bbm_amd.MaterialSet, name)).parameters["order"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "lanes"
    for name in ("gather", "scatter"):
        assert callable(getattr(bbm_amd.MaterialPlan, name))
    assert list(inspect.signature(bbm_amd.MaterialPlan.gather).parameters)[1:] == ["tensors", "mask", "stream"]
    assert list(inspect.signature(bbm_amd.MaterialPlan.scatter).parameters)[1:] == ["tensors", "out", "stream"]


def bare_plan(compact):
    """A MaterialPlan that owns nothing: what the keyword rules look at."""
    import bbm_amd
    p = object.__new__(bbm_amd.MaterialPlan)
    p._handle, p.compact = None, compact
    return p


def test_order_keyword_rules():
    import bbm_amd
    rule = bbm_amd.MaterialSet._sorted
    plain, compact = bare_plan(False), bare_plan(True)
    ids = object()
    assert rule("lanes", ids, None) is False and rule("lanes", None, plain) is False
    assert rule("plan", None, plain) is True and rule("plan", None, compact) is True
    with pytest.raises(ValueError, match='order="plan" needs plan='):
        rule("plan", None, None)
    with pytest.raises(ValueError, match='order="plan" needs plan='):
        rule("plan", ids, None)
    with pytest.raises(ValueError, match='order="plan" needs plan='):
        rule("plan", ids, plain)
    for bad in ("slots", "Plan", "", None, 1):
        with pytest.raises(ValueError, match="order: expected"):
            rule(bad, None, plain)
    with pytest.raises(ValueError, match="compact plan"):
        rule("lanes", None, compact)


def test_calls_apply_the_rules_before_the_library():
    """The calls themselves, on a set that owns nothing: the order= rules are reached after the normal's and the
    tangent's checks (the existing order) and before any handle is used."""
    import bbm_amd
    torch = pytest.importorskip("torch")
    s = object.__new__(bbm_amd.MaterialSet)
    s._handle = None
    d = torch.zeros((3, 8))
    xi = torch.zeros((2, 8))
    compact = bare_plan(True)
    for call in (lambda **kw: s.eval_pdf(d, d, **kw), lambda **kw: s.eval(d, d, **kw), lambda **kw: s.pdf(d, d, **kw),
                 lambda **kw: s.sample_eval(d, xi, **kw)):
        with pytest.raises(ValueError, match='order="plan" needs plan='):
            call(order="plan")
        with pytest.raises(ValueError, match='order="plan" needs plan='):
            call(order="plan", plan=bare_plan(False), material=object())
        with pytest.raises(ValueError, match="order: expected"):
            call(order="sorted", plan=bare_plan(False))
        with pytest.raises(ValueError, match="compact plan"):
            call(plan=compact)
        with pytest.raises(ValueError, match="compact plan"):
            call(plan=compact, order="lanes")
        # the frame's rules come first, as without order=
        with pytest.raises(ValueError, match="tangent= needs normal="):
            call(order="nonsense", tangent=d)
        with pytest.raises(TypeError, match="normal"):
            call(order="nonsense", normal=d.double())
