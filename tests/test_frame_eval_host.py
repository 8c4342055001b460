"""The world-space eval calls at the C-ABI boundary and the Python argument checks (CPU only, ctypes, nothing launched):
bbm_hip_eval_pdf_world / bbm_hip_eval_pdf_table_world are exported and bound, the ABI version and the registry are what
they were, every bad call is refused with its documented code before anything is launched, and the `normal=` /
`cosine=` keywords of eval_pdf / eval / pdf follow their rules: cosine without a normal and normal with varying are
ValueErrors, a bad normal is _normal_rows' TypeError or ValueError ahead of every other argument.  What needs a GPU is
in tests/test_gpu_frame_eval.py."""
import ctypes
import functools
import inspect
import os

import pytest

from tests import oracle_util as ou

torch = pytest.importorskip("torch")

N = 16
CT = [0.5, 0.5, 0.5, 0.1, 1.3]
SYMBOLS = ("bbm_hip_eval_pdf_world", "bbm_hip_eval_pdf_table_world")


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


def _world(lib, mid, p, k, n, normal=(1, 1, 1), in_=(1, 1, 1), out=(1, 1, 1), rgb=(1, 1, 1), pdf=1, cos=1):
    keep = []
    args = _ptrs(normal, keep) + _ptrs(in_, keep) + _ptrs(out, keep) + [None, n, 3, 0] + _ptrs(rgb, keep) + \
        _ptrs((pdf, cos), keep) + [None]
    return lib.bbm_hip_eval_pdf_world(mid, p, k, *args)


def test_symbols_exported_and_bound(lib):
    from bbm_amd import _lib
    header = open(os.path.join(ou.ROOT, "include", "bbm_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
        assert f"int {s}(" in header, s
        # one argument per parameter of the declaration: 3 head, 9 direction rows, mask, n, component, unit, 5 outputs,
        # the stream
        assert len(_lib.SIGNATURES[s][1]) == 22, s
        assert _lib.SIGNATURES[s][1][13] is ctypes.c_size_t, s


def test_abi_version_and_registry_unchanged(lib):
    from tests.test_abi import REGISTRY_ORDER
    assert lib.bbm_hip_abi_version() == 12
    assert lib.bbm_hip_num_models() == 49
    assert [lib.bbm_hip_model_name(i).decode() for i in range(49)] == REGISTRY_ORDER
    tables = [n for i, n in enumerate(REGISTRY_ORDER) if lib.bbm_hip_model_has_table(i) == 1]
    assert len(tables) == 43


def test_world_call_error_codes(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    # a bad id, a bad parameter count: ahead of the pointers
    assert _world(lib, 99, p, 5, N) == _lib.ERR_INVALID_MODEL
    assert _world(lib, 99, None, 4, N, normal=(0, 0, 0), in_=(0, 0, 0), out=(0, 0, 0)) == _lib.ERR_INVALID_MODEL
    assert _world(lib, ct | _lib.RUNTIME_AGGREGATE, p, 5, N) == _lib.ERR_INVALID_MODEL     # not a fused aggregate
    assert _world(lib, ct, p, 4, N) == _lib.ERR_INVALID_ARG
    assert b"expected 5 parameters" in lib.bbm_hip_last_error()
    assert _world(lib, ct | _lib.CALL_EXACT, p, 4, N) == _lib.ERR_INVALID_ARG
    # a NULL normal, in or out pointer
    for k in range(3):
        one = tuple(int(j != k) for j in range(3))
        assert _world(lib, ct, p, 5, N, normal=one) == _lib.ERR_INVALID_ARG, k
        assert b"normal direction pointer is NULL" in lib.bbm_hip_last_error()
        assert _world(lib, ct, p, 5, N, in_=one) == _lib.ERR_INVALID_ARG, k
        assert b"NULL" in lib.bbm_hip_last_error()
        assert _world(lib, ct, p, 5, N, out=one) == _lib.ERR_INVALID_ARG, k
        assert b"NULL" in lib.bbm_hip_last_error()
    # a partial r / g / b triple, with or without the pdf
    for group in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)):
        for pdf in (0, 1):
            assert _world(lib, ct, p, 5, N, rgb=group, pdf=pdf) == _lib.ERR_INVALID_ARG, (group, pdf)
            assert b"eval output pointer is NULL" in lib.bbm_hip_last_error()
    # no output at all: the cosine alone is not a mode
    for cos in (0, 1):
        assert _world(lib, ct, p, 5, N, rgb=(0, 0, 0), pdf=0, cos=cos) == _lib.ERR_INVALID_ARG, cos
        assert b"every output pointer is NULL" in lib.bbm_hip_last_error()


def test_world_call_n_zero_is_a_noop(lib):
    from bbm_amd import _lib
    p = (ctypes.c_float * 5)(*CT)
    ct = lib.bbm_hip_model_id(b"CookTorrance")
    none = dict(normal=(0, 0, 0), in_=(0, 0, 0), out=(0, 0, 0), rgb=(0, 0, 0), pdf=0, cos=0)
    assert _world(lib, ct, p, 5, 0, **none) == 0
    assert _world(lib, ct | _lib.CALL_EXACT, p, 5, 0, **none) == 0
    assert _world(lib, ct, p, 4, 0, **none) == _lib.ERR_INVALID_ARG           # the id and the count are still checked
    for name in ("He", "Merl", "Aggregate<Lambertian,Bagher>"):               # every row has the uniform call
        mid = lib.bbm_hip_model_id(name.encode())
        k = lib.bbm_hip_model_nparams(mid)
        q = (ctypes.c_float * max(k, 1))()
        assert _world(lib, mid, q, k, 0, **none) == 0, name


def test_table_world_call_on_null_table(lib):
    from bbm_amd import _lib
    for flags in (0, _lib.CALL_EXACT):
        for n in (0, N):
            assert lib.bbm_hip_eval_pdf_table_world(None, flags, None, *([None] * 10), n, 3, 0,
                                                    *([None] * 6)) == _lib.ERR_INVALID_ARG
            assert b"table is NULL" in lib.bbm_hip_last_error()


def test_python_surface_exists():
    import bbm_amd
    for cls in (bbm_amd.BsdfModel, bbm_amd.MaterialTable, bbm_amd.AggregateModel):
        sig = inspect.signature(cls.eval_pdf)
        for key, default in (("normal", None), ("cosine", False)):
            assert sig.parameters[key].default is default and \
                sig.parameters[key].kind is inspect.Parameter.KEYWORD_ONLY, (cls, key)
    assert "staged" in bbm_amd.AggregateModel.eval_pdf.__doc__


def _callers():
    """eval_pdf, eval and pdf of a model, a tree and a table, as f(in_, out, **kw); nothing here reaches the table
    handle, so a table without one stands for it."""
    import bbm_amd
    ct = bbm_amd.CookTorrance()
    tree = bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance())
    fns = [m_fn for m in (ct, tree) for m_fn in (m.eval_pdf, m.eval, m.pdf)]
    class Table(bbm_amd.MaterialTable):
        def __init__(self):
            self._handle = None
    t = Table()
    return fns + [functools.partial(f, material=None) for f in (t.eval_pdf, t.eval, t.pdf)]


def test_python_keyword_rules_before_any_launch():
    d = torch.zeros((3, N), dtype=torch.float32)
    f32 = torch.zeros((3, N), dtype=torch.float32)
    bad_normals = [
        (f32.double(), TypeError),                                  # float64: floatRGB only
        (f32.numpy(), TypeError),                                   # not a tensor
        (torch.zeros((N, 3), dtype=torch.float32), ValueError),     # shape
        (torch.zeros((3, N + 1), dtype=torch.float32), ValueError),  # length
        (torch.zeros((3, 2 * N), dtype=torch.float32)[:, ::2], ValueError),     # stride
        (f32, TypeError),                                           # device: a host tensor
    ]
    for fn in _callers():
        with pytest.raises(ValueError, match="cosine=True needs normal="):
            fn(d, d, cosine=True)
        for normal, exc in bad_normals:
            for cosine in (False, True):
                with pytest.raises(exc, match="normal"):
                    fn(d, d, normal=normal, cosine=cosine)
    # normal= with varying=: a ValueError that names to_local, whatever the normal is
    import bbm_amd
    ct = bbm_amd.CookTorrance()
    for fn in (ct.eval_pdf, ct.eval, ct.pdf):
        for normal in (f32, f32.double()):
            with pytest.raises(ValueError, match="to_local"):
                fn(d, d, normal=normal, varying={"roughness": torch.zeros(N)})
    tree = bbm_amd.AggregateModel(bbm_amd.Lambertian(), bbm_amd.CookTorrance())
    with pytest.raises(ValueError, match="to_local"):
        tree.eval_pdf(d, d, normal=f32, varying={})
    # normal=None, cosine=False stays today's path: the host tensors are refused by the checks of `in`
    for fn in (ct.eval_pdf, tree.eval_pdf):
        with pytest.raises(TypeError):
            fn(d, d, normal=None)
