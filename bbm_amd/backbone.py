"""Batched BSDF models over device memory -- the Python face of the HIP backbone.

Mirrors the reference's runtime model handle (bsdf_ptr, include/bbm/bsdf_ptr.h:21-165, exposed
to Python as BsdfPtr with eval / sample / pdf / reflectance, include/python/py_core.h:106-112),
but every call takes N direction pairs at once instead of one:

  * directions: a float32 CUDA tensor of shape (3, N) (rows x, y, z -- SoA) or a 3-tuple of
    1-D float32 CUDA tensors;
  * component / unit: bsdf_flag / unit_t, uniform per call (include/bbm/bsdf_flag.h,
    include/bbm/unit.h);
  * mask: optional bool/uint8 tensor of N lanes (the reference's `Mask mask=true`).

All work runs in libbbm_hip (hand-written gfx950 kernels) on the current torch stream; this
module only allocates outputs and passes pointers.  There is no CPU fallback.
"""
import copy
import ctypes
import enum
import re

import numpy as np

from . import _lib
from .models import AGGREGATES, ATTRIBUTES, aggregate_key, attr_size, nparams, to_string


class bsdf_flag(enum.IntFlag):
    """include/bbm/bsdf_flag.h:21-27"""
    None_ = 0
    Diffuse = 1
    Specular = 2
    All = 3


class unit_t(enum.IntEnum):
    """include/bbm/unit.h:20-24"""
    Radiance = 0
    Importance = 1


class BsdfSample:
    """bsdfsample (include/bbm/bsdfsample.h:20-25), batched: direction (3, N), pdf (N,), flag (N,)."""

    def __init__(self, direction, pdf, flag):
        self.direction, self.pdf, self.flag = direction, pdf, flag


def _torch():
    import torch
    return torch


def _is_f64(t):
    """True if the direction rows are float64 (the doubleRGB configuration)."""
    torch = _torch()
    rows = list(t) if isinstance(t, (tuple, list)) else [t]
    return bool(rows) and isinstance(rows[0], torch.Tensor) and rows[0].dtype == torch.float64


def _soa(t, n=None, what="direction", dtype=None):
    """Return (x_ptr, y_ptr, z_ptr, n) for a (3, N) tensor or a tuple of three 1-D tensors of `dtype`
    (float32 unless given)."""
    torch = _torch()
    dtype = torch.float32 if dtype is None else dtype
    if isinstance(t, (tuple, list)):
        rows = list(t)
    else:
        if t.dim() != 2 or t.shape[0] != 3:
            raise ValueError(f"{what}: expected a (3, N) tensor, got {tuple(t.shape)}")
        rows = [t[0], t[1], t[2]]
    for r in rows:
        if not isinstance(r, torch.Tensor) or r.dtype != dtype or not r.is_cuda:
            raise TypeError(f"{what}: expected {str(dtype).replace('torch.', '')} CUDA tensors")
        if r.dim() != 1 or r.stride(0) != 1:
            raise ValueError(f"{what}: rows must be contiguous 1-D tensors")
    m = rows[0].numel()
    if any(r.numel() != m for r in rows):
        raise ValueError(f"{what}: x/y/z lengths differ")
    if n is not None and m != n:
        raise ValueError(f"{what}: expected {n} elements, got {m}")
    return rows[0].data_ptr(), rows[1].data_ptr(), rows[2].data_ptr(), m


def _mask_ptr(mask, n):
    if mask is None:
        return None, None
    torch = _torch()
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if mask.dtype != torch.uint8 or not mask.is_cuda or mask.numel() != n:
        raise TypeError("mask: expected a bool/uint8 CUDA tensor with one entry per pair")
    mask = mask.contiguous()
    return mask.data_ptr(), mask


def _out_rows(t, rows, n, device, what, dtype=None):
    """Validate a caller-supplied output buffer before its row pointers reach a kernel: float32 (or `dtype`), on
    the inputs' device, shape (rows, n) (or (n,) for rows == 0) with every row contiguous."""
    torch = _torch()
    dtype = torch.float32 if dtype is None else dtype
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{what}: expected a {str(dtype).replace('torch.', '')} CUDA tensor")
    if not t.is_cuda or t.device != device:
        raise ValueError(f"{what}: must live on {device}, got {t.device}")
    shape = (n,) if rows == 0 else (rows, n)
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: expected shape {shape}, got {tuple(t.shape)}")
    if t.stride(-1) != 1:
        raise ValueError(f"{what}: rows must be contiguous")
    return t


def _stream_ptr(stream):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


def _on_stream(stream, *tensors):
    """Tensors allocated here (outputs, the mask copy) but used by a launch on a stream other than the current
    one: tell the caching allocator, so their memory is not reused before that stream has run the kernel."""
    if stream is None:
        return
    torch = _torch()
    if stream == torch.cuda.current_stream():
        return
    for t in tensors:
        if t is not None:
            t.record_stream(stream)


def _sample_eval_inputs(out, xi):
    """sample_eval's inputs, checked before anything is allocated or launched: (out's x, y, z pointers, n, the two
    xi rows).  floatRGB only: float64 tensors are a TypeError, as for `varying=`."""
    torch = _torch()
    if _is_f64(out) or _is_f64(xi):
        raise TypeError("sample_eval: floatRGB only (float32 tensors)")
    ox, oy, oz, n = _soa(out, what="out")
    if isinstance(xi, (tuple, list)):
        if len(xi) != 2:
            raise ValueError("xi: expected two rows")
        x0, x1 = xi
    else:
        if not isinstance(xi, torch.Tensor) or xi.dim() != 2 or xi.shape[0] != 2:
            raise ValueError("xi: expected a (2, N) tensor")
        x0, x1 = xi[0], xi[1]
    for x in (x0, x1):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.numel() != n or \
                x.dim() != 1 or (n > 1 and x.stride(0) != 1):
            raise TypeError("xi: expected float32 CUDA rows with one entry per direction")
    return ox, oy, oz, n, x0, x1


def _lanes(t):
    """The lane count a direction argument seems to have (a (3, N) tensor or three rows), or None: for checks that
    run before that argument's own."""
    torch = _torch()
    t = t[0] if isinstance(t, (tuple, list)) and len(t) > 0 else t
    return int(t.shape[-1]) if isinstance(t, torch.Tensor) and t.dim() >= 1 else None


def _normal_rows(normal, like, what="normal"):
    """The shading normals of the world-space calls, checked before anything else is: a (3, N) float32 CUDA tensor
    with contiguous rows, one normal per lane of `like` -> its three row pointers.  Wrong dtype (float64 included) or
    device: TypeError; wrong shape, length or stride: ValueError."""
    torch = _torch()
    if not isinstance(normal, torch.Tensor) or normal.dtype != torch.float32:
        raise TypeError(f"{what}: floatRGB only, expected a (3, N) float32 CUDA tensor")
    if normal.dim() != 2 or normal.shape[0] != 3:
        raise ValueError(f"{what}: expected a (3, N) tensor, got {tuple(normal.shape)}")
    n = _lanes(like)
    if n is not None and normal.shape[1] != n:
        raise ValueError(f"{what}: expected {n} normals, got {normal.shape[1]}")
    if normal.shape[1] > 1 and normal.stride(1) != 1:
        raise ValueError(f"{what}: rows must be contiguous")
    if not normal.is_cuda:
        raise TypeError(f"{what}: expected a CUDA tensor, got one on {normal.device}")
    first = like[0] if isinstance(like, (tuple, list)) and len(like) > 0 else like
    if isinstance(first, torch.Tensor) and first.is_cuda and first.device != normal.device:
        raise TypeError(f"{what}: must live on {first.device}, got {normal.device}")
    return normal[0].data_ptr(), normal[1].data_ptr(), normal[2].data_ptr()


def _frame_rows(normal, tangent, like):
    """normal= and tangent= of a world-space call, checked before anything else is (the tangent right after the
    normal, by the same code): None for the local call, the normal's three row pointers, or those and the tangent's
    three.  A tangent needs a normal: it fills the X and Y of the normal's frame."""
    if normal is None:
        if tangent is not None:
            raise ValueError("tangent= needs normal=: the tangent fills X and Y of the shading normal's frame")
        return None
    nptr = _normal_rows(normal, like)
    return nptr if tangent is None else nptr + _normal_rows(tangent, like, what="tangent")


def _frame_fn(name, fptr):
    """The C-ABI call `name` for the frame pointers of _frame_rows: its *_tangent form where they hold a tangent."""
    return getattr(_lib.load(), name + "_tangent" if fptr is not None and len(fptr) == 6 else name)


def _frame6(fptr):
    """The frame pointers of _frame_rows as the six the *_sorted calls take: normal, then tangent, NULL where absent."""
    return tuple(fptr or ()) + (None,) * (6 - len(fptr or ()))


def _world_normal(normal, cosine, varying, in_, out, tangent=None):
    """The world-space keywords of eval_pdf, checked ahead of every other argument: the frame's row pointers
    (_frame_rows), or None for the local call.  cosine and tangent need a normal; normal= excludes varying= and float64
    directions."""
    if normal is None:
        if tangent is not None:
            _frame_rows(normal, tangent, in_)
        if cosine:
            raise ValueError("cosine=True needs normal=: the cosine is that of `in` against the shading normal")
        return None
    if varying is not None:
        raise ValueError("normal= with varying=: there is no world-space call over per-lane parameters; "
                         "take the directions through to_local(normal, .) and use the local call")
    nptr = _frame_rows(normal, tangent, in_)
    if _is_f64(in_) or _is_f64(out):
        raise TypeError("normal: the world-space calls are floatRGB only (float32 directions)")
    return nptr


def _with_cosine(result, k, cosine):
    """eval / pdf: element k of eval_pdf's result, and its cosine (the last element) where that was asked for."""
    return (result[k], result[-1]) if cosine else result[k]


def _frame_call(fn_name, normal, v, mask, stream, tangent=None):
    torch = _torch()
    nptr = _frame_rows(normal, tangent, v)
    if _is_f64(v):
        raise TypeError("shading frames: floatRGB only (float32 tensors)")
    x, y, z, n = _soa(v, what="v")
    mptr, _keep = _mask_ptr(mask, n)
    r = torch.empty((3, n), dtype=torch.float32, device=_device(v))
    _on_stream(stream, _keep, r)
    _lib.check(_frame_fn(fn_name, nptr)(*nptr, x, y, z, mptr, n, r[0].data_ptr(), r[1].data_ptr(),
                                              r[2].data_ptr(), _stream_ptr(stream)))
    return r


def to_local(normal, v, mask=None, *, stream=None, tangent=None):
    """World-space vectors v (3, N) in the shading frame of one normal per lane (bbm_hip_frame_to_local): the
    reference's toLocalShadingFrame, transpose(toGlobalShadingFrame(normal)) v.  normal: (3, N) float32, any length
    per normal; a lane whose normal is (about) zero, and a lane with mask == 0, gets (0, 0, 0).  -> (3, N).
    tangent: (3, N) float32 world-space tangents, any length (bbm_hip_frame_to_local_tangent): X is the tangent's part
    perpendicular to the normal, normalized, and Y = Z x X; a lane whose tangent has no such part (zero, parallel to the
    normal, NaN) keeps the normal-only frame."""
    return _frame_call("bbm_hip_frame_to_local", normal, v, mask, stream, tangent)


def to_global(normal, v, mask=None, *, stream=None, tangent=None):
    """Local vectors v (3, N) in world space (bbm_hip_frame_to_global): toGlobalShadingFrame(normal) v; see to_local."""
    return _frame_call("bbm_hip_frame_to_global", normal, v, mask, stream, tangent)


def _device(t):
    """The device of a (3, N) tensor or of a tuple of rows."""
    return (t[0] if isinstance(t, (tuple, list)) else t).device


def _xi_rows(xi, n, dtype):
    """sample's two xi rows of `dtype`, from a (2, N) tensor or a pair of rows, one entry per direction."""
    if isinstance(xi, (tuple, list)):
        x0, x1 = xi
    else:
        if xi.dim() != 2 or xi.shape[0] != 2:
            raise ValueError("xi: expected a (2, N) tensor")
        x0, x1 = xi[0], xi[1]
    for x in (x0, x1):
        if x.dtype != dtype or not x.is_cuda or x.numel() != n or x.stride(0) != 1:
            raise TypeError(f"xi: expected {str(dtype).replace('torch.', '')} CUDA rows with one entry per direction")
    return x0, x1


def _eval_pdf_outputs(mode, n, device, rgb, pdf):
    """eval_pdf's (rgb, pdf) for the outputs `mode` asks for (1: rgb, 2: pdf): allocated, or the caller's buffer
    validated; an output that is not asked for is passed through."""
    torch = _torch()
    if mode & 1:
        rgb = torch.empty((3, n), dtype=torch.float32, device=device) if rgb is None else \
            _out_rows(rgb, 3, n, device, "rgb")
    if mode & 2:
        pdf = torch.empty((n,), dtype=torch.float32, device=device) if pdf is None else \
            _out_rows(pdf, 0, n, device, "pdf")
    return rgb, pdf


def _eval_pdf_ptrs(mode, rgb, pdf):
    """The r, g, b and pdf pointers of the calls that take the mode from their outputs: NULL where not asked for."""
    return (*_row_ptrs(rgb if mode & 1 else None), pdf.data_ptr() if mode & 2 else None)


def _sample_outputs(n, device, dtype):
    """(direction, pdf, flag) for one sample call."""
    torch = _torch()
    return (torch.empty((3, n), dtype=dtype, device=device), torch.empty((n,), dtype=dtype, device=device),
            torch.empty((n,), dtype=torch.int32, device=device))


def _sample_eval_outputs(n, device, value, weight):
    """(direction, pdf, flag, value or None, weight or None) for one sample_eval call."""
    torch = _torch()
    d, p, f = _sample_outputs(n, device, torch.float32)
    v = torch.empty((3, n), dtype=torch.float32, device=device) if value else None
    w = torch.empty((3, n), dtype=torch.float32, device=device) if weight else None
    return d, p, f, v, w


def _row_ptrs(t):
    """The three row pointers of a (3, N) output, or three NULLs for a group that is not stored."""
    return (None, None, None) if t is None else (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def _weight(value, direction, pdf):
    """sample_eval's weight with torch float32 ops: value * direction_z / pdf where pdf > epsilon(float32), else 0."""
    torch = _torch()
    eps = float(np.finfo(np.float32).eps)
    return torch.where(pdf > eps, (value * direction[2]) / pdf, torch.zeros_like(value))


def model_names():
    """Models available in the loaded HIP library (BBM_EXPORT_BSDFMODEL registry equivalent)."""
    lib = _lib.load()
    return [lib.bbm_hip_model_name(i).decode() for i in range(lib.bbm_hip_num_models())]


def _model_params(model_id, which):
    lib = _lib.load()
    k = _lib.check(lib.bbm_hip_model_nparams(model_id))
    buf = (ctypes.c_float * max(k, 1))()
    _lib.check(lib.bbm_hip_model_params(model_id, which, buf, k))
    return np.array(buf[:k], dtype=np.float32)


class BsdfModel:
    """One parameterised BSDF model, evaluated in batches on the GPU."""

    def __init__(self, name, *args, **kwargs):
        lib = _lib.load()
        if name not in ATTRIBUTES and name not in AGGREGATES:
            raise ValueError(f"unknown BSDF model: {name}")
        mid = lib.bbm_hip_model_id(name.encode())
        if mid < 0:
            raise _lib.BackboneError(mid, f"model {name} is not available in libbbm_hip")
        self.name = name
        self.model_id = mid
        self._params = _model_params(mid, 0)
        if name in AGGREGATES:
            # Aggregate(child, child): children given as models (aggregatemodel.h:33, aggregate() :232-233)
            if kwargs or (args and len(args) != len(AGGREGATES[name])):
                raise TypeError(f"{name}: expected {len(AGGREGATES[name])} child models")
            k = 0
            for c, child in zip(AGGREGATES[name], args):
                if child.name != c:
                    raise TypeError(f"{name}: expected a {c} child, got {child.name}")
                self._params[k:k + child._params.size] = child._params
                k += child._params.size
            return
        layout = ATTRIBUTES[name]
        if len(args) > len(layout):
            raise TypeError(f"{name}: too many positional attributes")
        values = dict(zip([a for a, _ in layout], args))
        for k, v in kwargs.items():
            if k not in dict(layout):
                raise TypeError(f"{name}: unknown attribute '{k}'")
            if k in values:
                raise TypeError(f"{name}: attribute '{k}' given twice")
            values[k] = v
        for k, v in values.items():
            self.set_attribute(k, v)

    @property
    def runtime(self):
        """A fused Aggregate(A, B) evaluated as the reference's runtime aggregatebsdf (what fromString / bsdf_import
        build, include/bbm/aggregatebsdf.h) rather than as aggregatemodel<A, B>: the model id carries
        BBM_HIP_RUNTIME_AGGREGATE."""
        return self.model_id >= 0 and bool(self.model_id & _lib.RUNTIME_AGGREGATE)

    # ---------------------------------------------------------------- attributes
    def _slot(self, attr):
        k = 0
        for a, shape in ATTRIBUTES[self.name]:
            if a == attr:
                return k, shape
            k += attr_size(shape)
        raise KeyError(attr)

    def set_attribute(self, attr, value):
        k, shape = self._slot(attr)
        n = attr_size(shape)
        src = np.asarray(value, dtype=np.float64).reshape(-1)
        with np.errstate(over="ignore"):
            v = src.astype(np.float32)
        if np.any(np.isfinite(src) & ~np.isfinite(v)):
            # the reference's string conversion refuses a value beyond the float range (std::out_of_range)
            raise ValueError(f"{self.name}.{attr}: value out of the float range: {src[np.isfinite(src) & ~np.isfinite(v)]}")
        if v.size == 1 and n > 1:      # a scalar broadcasts over an RGB / Vec2d attribute
            v = np.repeat(v, n)
        if v.size != n:
            raise ValueError(f"{self.name}.{attr}: expected {n} values, got {v.size}")
        self._params[k:k + n] = v

    def attribute(self, attr):
        k, shape = self._slot(attr)
        v = self._params[k:k + attr_size(shape)].copy()
        return v[0] if shape == () else v.reshape(shape)

    def parameter_values(self, flag=None):
        """Flat parameter vector (bbm::parameter_values, include/bbm/bsdf_enumerate.h:103-131).
        flag=None: every parameter (the layout the kernels take, Dependent ones included);
        flag=bsdf_attr bits: only the parameters whose attribute flags intersect it (the reference's
        default bsdf_attr::All = 0x0F leaves out Dependent attributes)."""
        if flag is None:
            return self._params.copy()
        return self._params[self.parameter_indices(flag)].copy()

    def parameter_attrs(self):
        """Per-parameter bsdf_attr flags (bbm_hip_model_param_attrs)."""
        lib = _lib.load()
        k = self._params.size
        buf = (ctypes.c_uint32 * max(k, 1))()
        _lib.check(lib.bbm_hip_model_param_attrs(self.model_id, buf, k))
        return np.array(buf[:k], dtype=np.uint32)

    def parameter_indices(self, flag=0x0F):
        """Indices into the full parameter vector selected by parameter_values(flag)."""
        return np.nonzero(self.parameter_attrs() & np.uint32(flag))[0]

    def children(self):
        """Aggregate: the child models (copies); otherwise []."""
        if self.name not in AGGREGATES:
            return []
        out, k = [], 0
        for c in AGGREGATES[self.name]:
            m = BsdfModel(c)
            m._params[:] = self._params[k:k + m._params.size]
            k += m._params.size
            out.append(m)
        return out

    def set_parameter_values(self, values):
        v = np.asarray(values, dtype=np.float32).reshape(-1)
        if v.size != self._params.size:
            raise ValueError(f"{self.name}: expected {self._params.size} parameters, got {v.size}")
        self._params[:] = v

    def parameter_default_values(self):
        return _model_params(self.model_id, 0)

    def parameter_lower_bound(self):
        return _model_params(self.model_id, 1)

    def parameter_upper_bound(self):
        return _model_params(self.model_id, 2)

    def __str__(self):
        return to_string(self.name, self._params)

    __repr__ = __str__

    # ---------------------------------------------------------------- batched evaluation
    def _call_id(self, exact):
        """The model id for one call: exact=None follows set_exact_subnormals (the process-wide default), True / False
        force exact / default mode for this call only (BBM_HIP_CALL_EXACT / BBM_HIP_CALL_DEFAULT, re-entrant)."""
        if exact is None:
            return self.model_id
        return self.model_id | (_lib.CALL_EXACT if exact else _lib.CALL_DEFAULT)

    def _pptr(self):
        return self._params.ctypes.data_as(ctypes.c_void_p)

    def has_f64(self):
        """True if the model has doubleRGB kernels (bbm_hip_model_has_f64)."""
        return _lib.check(_lib.load().bbm_hip_model_has_f64(self.model_id)) == 1

    def has_varying(self):
        """True if the model has per-lane parameter kernels (bbm_hip_model_has_varying): the `varying=` keyword of
        eval / pdf / eval_pdf / sample / reflectance."""
        return _lib.check(_lib.load().bbm_hip_model_has_varying(self.model_id)) == 1

    @property
    def anisotropic(self):
        """Whether the model's parameters run along the shading frame's X and Y (bbm_hip_model_anisotropic): the
        models for which tangent= of the world-space calls turns the lobe."""
        return bool(_lib.check(_lib.load().bbm_hip_model_anisotropic(self.model_id)))

    def has_table(self):
        """True if the model can be held in a MaterialTable (bbm_hip_model_has_table)."""
        return _lib.check(_lib.load().bbm_hip_model_has_table(self.model_id)) == 1

    def _varying(self, varying, n, device, f64=False):
        """The `varying=` mapping as bbm_hip_*_varying's host array of row pointers: (ctypes array of nparams
        pointers, the row tensors to keep alive).  Keys: an attribute name (single models) or an integer parameter
        index (the only form for fused aggregates); values: float32 CUDA tensors of shape (n,) for one slot or (k, n)
        with unit-stride rows for a k-slot attribute.  Raises before anything is launched."""
        torch = _torch()
        if f64:
            raise TypeError("varying: per-lane parameters are floatRGB only (float32 tensors)")
        total = self._params.size
        rows = [None] * total
        for key, t in dict(varying).items():
            if isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                first, count = int(key), 1
                if not 0 <= first < total:
                    raise ValueError(f"{self.name}: varying index {first} out of range [0, {total})")
            else:
                if self.name not in ATTRIBUTES or key not in dict(ATTRIBUTES[self.name]):
                    raise TypeError(f"{self.name}: unknown attribute '{key}'")
                first, shape = self._slot(key)
                count = attr_size(shape)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != device:
                raise TypeError(f"{self.name}: varying[{key!r}]: expected a float32 CUDA tensor on {device}")
            if t.dim() == 1 and count == 1:
                got = [t]
            elif t.dim() == 2 and t.shape[0] == count:
                got = [t[j] for j in range(count)]
            else:
                want = f"({n},)" if count == 1 else f"({count}, {n})"
                raise ValueError(f"{self.name}: varying[{key!r}]: expected shape {want}, got {tuple(t.shape)}")
            for j, r in enumerate(got):
                if r.numel() != n:
                    raise ValueError(f"{self.name}: varying[{key!r}]: expected {n} lanes, got {r.numel()}")
                if n > 1 and r.stride(0) != 1:
                    raise ValueError(f"{self.name}: varying[{key!r}]: rows must have unit stride")
                if rows[first + j] is not None:
                    raise ValueError(f"{self.name}: parameter {first + j} given twice in varying")
                rows[first + j] = r
        arr = (ctypes.c_void_p * max(total, 1))(*[None if r is None else r.data_ptr() for r in rows])
        return arr, [r for r in rows if r is not None]

    def _params_f64(self, params64):
        if params64 is None:
            return np.ascontiguousarray(self._params, dtype=np.float64)
        v = np.ascontiguousarray(params64, dtype=np.float64).reshape(-1)
        if v.size != self._params.size:
            raise ValueError(f"{self.name}: expected {self._params.size} parameters, got {v.size}")
        return v

    def _eval_pdf_f64(self, in_, out, component, unit, mask, rgb, pdf, stream, params64):
        """doubleRGB (Value = double): float64 directions -> float64 eval RGB and pdf (bbm_hip_eval_pdf_f64).
        Parameters: params64 if given, else the model's (float) parameter vector widened to double."""
        torch = _torch()
        f64 = torch.float64
        ix, iy, iz, n = _soa(in_, what="in", dtype=f64)
        ox, oy, oz, _ = _soa(out, n, what="out", dtype=f64)
        mptr, _keep = _mask_ptr(mask, n)
        dev = torch.device("cuda", torch.cuda.current_device())
        rgb = torch.empty((3, n), dtype=f64, device=dev) if rgb is None else _out_rows(rgb, 3, n, dev, "rgb", f64)
        pdf = torch.empty((n,), dtype=f64, device=dev) if pdf is None else _out_rows(pdf, 0, n, dev, "pdf", f64)
        p = self._params_f64(params64)
        _on_stream(stream, _keep, rgb, pdf)
        _lib.check(_lib.load().bbm_hip_eval_pdf_f64(
            self.model_id, p.ctypes.data_as(ctypes.c_void_p), p.size, ix, iy, iz, ox, oy, oz, mptr, n, int(component),
            int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(), pdf.data_ptr(), _stream_ptr(stream)))
        return rgb, pdf

    def eval_pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *,
                 rgb=None, pdf=None, stream=None, mode=3, params64=None, exact=None, varying=None, normal=None,
                 cosine=False, tangent=None):
        """varying: per-lane parameters, {attribute name or parameter index: float32 CUDA rows} (_varying); lane i
        then evaluates the model with those parameters replaced by row[i] (bbm_hip_eval_pdf_varying).
        normal: a (3, N) float32 tensor of shading normals selects the world-space call (bbm_hip_eval_pdf_world):
        `in_` and `out` are in world space, and the result is what to_local(normal, in_), to_local(normal, out) and
        this call give in sequence, in one launch.  cosine=True (with normal=): the result gains a last element, the
        (N,) cosine of `in_` against the normal (the z of to_local(normal, in_)).  floatRGB only, not with varying=.
        tangent (with normal=): a (3, N) float32 tensor of world-space tangents, any length; for an anisotropic model
        (self.anisotropic) the frame's X follows it (bbm_hip_eval_pdf_world_tangent; to_local's tangent=), so the x / y
        roughness runs along the surface's own direction.  Any other model ignores it."""
        torch = _torch()
        nptr = _world_normal(normal, cosine, varying, in_, out, tangent)
        if varying is not None and _is_f64(in_):
            raise TypeError("varying: per-lane parameters are floatRGB only (float32 tensors)")
        if _is_f64(in_):
            rgb, pdf = self._eval_pdf_f64(in_, out, component, unit, mask, rgb if mode & 1 else None,
                                          pdf if mode & 2 else None, stream, params64)
            return (rgb if mode & 1 else None), (pdf if mode & 2 else None)
        ix, iy, iz, n = _soa(in_, what="in")
        ox, oy, oz, _ = _soa(out, n, what="out")
        mptr, _keep = _mask_ptr(mask, n)
        dev = torch.device("cuda", torch.cuda.current_device())
        rgb, pdf = _eval_pdf_outputs(mode, n, dev, rgb, pdf)
        lib = _lib.load()
        s = _stream_ptr(stream)
        _on_stream(stream, _keep, rgb, pdf)
        mid = self._call_id(exact)
        if nptr is not None:
            cos = torch.empty((n,), dtype=torch.float32, device=dev) if cosine else None
            _on_stream(stream, cos)
            _lib.check(_frame_fn("bbm_hip_eval_pdf_world", nptr)(
                mid, self._pptr(), self._params.size, *nptr, ix, iy, iz, ox, oy, oz, mptr, n, int(component), int(unit),
                *_eval_pdf_ptrs(mode, rgb, pdf), None if cos is None else cos.data_ptr(), s))
            return (rgb, pdf, cos) if cosine else (rgb, pdf)
        if varying is not None:
            vptr, vrows = self._varying(varying, n, _device(in_))
            _on_stream(stream, *vrows)
            _lib.check(lib.bbm_hip_eval_pdf_varying(
                mid, self._pptr(), self._params.size, vptr, ix, iy, iz, ox, oy, oz, mptr, n, int(component), int(unit),
                *_eval_pdf_ptrs(mode, rgb, pdf), s))
            return rgb, pdf
        if mode == 3:
            rc = lib.bbm_hip_eval_pdf(mid, self._pptr(), self._params.size, ix, iy, iz, ox, oy, oz, mptr, n,
                                      int(component), int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(),
                                      rgb[2].data_ptr(), pdf.data_ptr(), s)
        elif mode == 1:
            rc = lib.bbm_hip_eval(mid, self._pptr(), self._params.size, ix, iy, iz, ox, oy, oz, mptr, n,
                                  int(component), int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(), s)
        else:
            rc = lib.bbm_hip_pdf(mid, self._pptr(), self._params.size, ix, iy, iz, ox, oy, oz, mptr, n,
                                 int(component), int(unit), pdf.data_ptr(), s)
        _lib.check(rc)
        return rgb, pdf

    def eval(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        """Spectrum eval(in, out, component, unit, mask) for N pairs -> (3, N) RGB; with normal= and cosine=True
        (eval_pdf) -> (RGB, cosine)."""
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=1, **kw), 0, kw.get("cosine", False))

    def pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        """Value pdf(in, out, component, unit, mask) for N pairs -> (N,); with normal= and cosine=True (eval_pdf)
        -> (pdf, cosine)."""
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=2, **kw), 1, kw.get("cosine", False))

    def sample(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, stream=None,
               params64=None, exact=None, varying=None):
        """BsdfSample sample(out, xi, component, unit, mask) for N (out, xi) -> BsdfSample (float64 out / xi: the
        doubleRGB kernels, float64 direction and pdf).  exact, varying: as eval_pdf."""
        torch = _torch()
        f64 = _is_f64(out)
        dt = torch.float64 if f64 else torch.float32
        ox, oy, oz, n = _soa(out, what="out", dtype=dt)
        x0, x1 = _xi_rows(xi, n, dt)
        mptr, _keep = _mask_ptr(mask, n)
        dev = x0.device
        d, p, f = _sample_outputs(n, dev, dt)
        _on_stream(stream, _keep, d, p, f)
        lib = _lib.load()
        if varying is not None:
            vptr, vrows = self._varying(varying, n, dev, f64=f64)
            _on_stream(stream, *vrows)
            _lib.check(lib.bbm_hip_sample_varying(
                self._call_id(exact), self._pptr(), self._params.size, vptr, ox, oy, oz, x0.data_ptr(), x1.data_ptr(),
                mptr, n, int(component), int(unit), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(),
                f.data_ptr(), _stream_ptr(stream)))
            return BsdfSample(d, p, f)
        if f64:
            prm = self._params_f64(params64)
            fn, pp, npar = lib.bbm_hip_sample_f64, prm.ctypes.data_as(ctypes.c_void_p), prm.size
        else:
            fn, pp, npar = lib.bbm_hip_sample, self._pptr(), self._params.size
        _lib.check(fn(self._call_id(exact), pp, npar, ox, oy, oz, x0.data_ptr(), x1.data_ptr(), mptr, n, int(component),
                      int(unit), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(), f.data_ptr(),
                      _stream_ptr(stream)))
        return BsdfSample(d, p, f)

    def sample_eval(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, value=True,
                    weight=True, stream=None, exact=None, normal=None, tangent=None):
        """One BSDF call per bounce in one launch (bbm_hip_sample_eval): -> (BsdfSample, value, weight).  The sample is
        sample(out, xi)'s, value (3, N) is eval_pdf(sample.direction, out)[0] and weight (3, N) is
        value * direction_z / pdf where pdf > epsilon(float32), else 0 -- each bit for bit what the staged calls give,
        without the sampled direction's round trip through memory.  value=False / weight=False: that group is not
        stored and None is returned for it.  floatRGB only.
        normal: a (3, N) float32 tensor of shading normals selects the world-space call (bbm_hip_sample_eval_world):
        `out` and the returned direction are in world space, everything else is what to_local(normal, out), this call
        and to_global(normal, direction) give in sequence (the weight's cosine is the local direction's).
        tangent (with normal=): as eval_pdf's (bbm_hip_sample_eval_world_tangent)."""
        nptr = _frame_rows(normal, tangent, out)
        ox, oy, oz, n, x0, x1 = _sample_eval_inputs(out, xi)
        mptr, _keep = _mask_ptr(mask, n)
        outs = _sample_eval_outputs(n, x0.device, value, weight)
        _on_stream(stream, _keep, *outs)
        d, p, f, v, w = outs
        lib = _lib.load()
        fn, pre = (lib.bbm_hip_sample_eval, ()) if nptr is None else (_frame_fn("bbm_hip_sample_eval_world", nptr), nptr)
        _lib.check(fn(
            self._call_id(exact), self._pptr(), self._params.size, *pre, ox, oy, oz, x0.data_ptr(), x1.data_ptr(), mptr, n,
            int(component), int(unit), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(), f.data_ptr(),
            *_row_ptrs(v), *_row_ptrs(w), _stream_ptr(stream)))
        return BsdfSample(d, p, f), v, w

    def reflectance(self, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, stream=None,
                    params64=None, exact=None, varying=None):
        """Spectrum reflectance(out, component, unit, mask) for N directions -> (3, N) RGB (float64 directions:
        the doubleRGB kernels, float64 RGB).  varying: as eval_pdf."""
        torch = _torch()
        if varying is not None and _is_f64(out):
            raise TypeError("varying: per-lane parameters are floatRGB only (float32 tensors)")
        if _is_f64(out):
            ox, oy, oz, n = _soa(out, what="out", dtype=torch.float64)
            mptr, _keep = _mask_ptr(mask, n)
            dev = _device(out)
            rgb = torch.empty((3, n), dtype=torch.float64, device=dev)
            p = self._params_f64(params64)
            _on_stream(stream, _keep, rgb)
            _lib.check(_lib.load().bbm_hip_reflectance_f64(
                self.model_id, p.ctypes.data_as(ctypes.c_void_p), p.size, ox, oy, oz, mptr, n, int(component),
                int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(), _stream_ptr(stream)))
            return rgb
        ox, oy, oz, n = _soa(out, what="out")
        mptr, _keep = _mask_ptr(mask, n)
        dev = _device(out)
        rgb = torch.empty((3, n), dtype=torch.float32, device=dev)
        _on_stream(stream, _keep, rgb)
        lib = _lib.load()
        if varying is not None:
            vptr, vrows = self._varying(varying, n, dev)
            _on_stream(stream, *vrows)
            _lib.check(lib.bbm_hip_reflectance_varying(
                self._call_id(exact), self._pptr(), self._params.size, vptr, ox, oy, oz, mptr, n, int(component),
                int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(), _stream_ptr(stream)))
            return rgb
        _lib.check(lib.bbm_hip_reflectance(self._call_id(exact), self._pptr(), self._params.size, ox, oy, oz, mptr, n,
                                           int(component), int(unit), rgb[0].data_ptr(), rgb[1].data_ptr(),
                                           rgb[2].data_ptr(), _stream_ptr(stream)))
        return rgb


# ------------------------------------------------------------------------- string import

_TOKEN = re.compile(r"\s*([A-Za-z_][A-Za-z0-9_]*|[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?|[()\[\],=])")


def _tokenize(s):
    pos, out = 0, []
    s = s.strip()
    while pos < len(s):
        m = _TOKEN.match(s, pos)
        if not m:
            raise ValueError(f"cannot parse BSDF string at: {s[pos:]!r}")
        out.append(m.group(1))
        pos = m.end()
    return out


def _parse_value(tok, i):
    if tok[i] == "[":
        vals, i = [], i + 1
        while tok[i] != "]":
            v, i = _parse_value(tok, i)
            vals.append(v)
            if tok[i] == ",":
                i += 1
        return vals, i + 1
    return float(tok[i]), i + 1


def _parse_model(tok, i, s):
    """Parse `Name(...)` starting at tok[i]; returns (model, next index)."""
    name = tok[i]
    if name == "Aggregate":
        # Aggregate(child, child) (aggregatemodel.h:184-212)
        if i + 1 >= len(tok) or tok[i + 1] != "(":
            raise ValueError(f"malformed BSDF string: {s!r}")
        kids, i = [], i + 2
        while tok[i] != ")":
            m, i = _parse_model(tok, i, s)
            kids.append(m)
            if tok[i] == ",":
                i += 1
        # the runtime aggregate: fromString<bsdf_ptr> maps "Aggregate" to aggregatebsdf (bsdf_string_convert.h:59)
        return Aggregate(*kids, runtime=True), i + 1
    if name not in ATTRIBUTES:
        raise ValueError(f"unknown BSDF model: {name}")
    m = BsdfModel(name)
    if i + 1 >= len(tok) or tok[i + 1] != "(":
        return m, i + 1
    i, layout, pos_idx = i + 2, [a for a, _ in ATTRIBUTES[name]], 0
    while tok[i] != ")":
        if i + 1 < len(tok) and tok[i + 1] == "=":
            attr = tok[i]
            v, i = _parse_value(tok, i + 2)
        else:
            attr = layout[pos_idx]
            v, i = _parse_value(tok, i)
        pos_idx += 1
        m.set_attribute(attr, np.asarray(v, dtype=np.float64))
        if tok[i] == ",":
            i += 1
    return m, i + 1


def fromString(s):
    """Construct a model from its bbm::toString form, e.g. 'CookTorrance(albedo = [0.5, 0.5, 0.5],
    roughness = 0.1, eta = 1.3)' or 'Aggregate(Lambertian(...), Bagher(...))'
    (bsdf_string_convert.h:52-82 / bsdf_import.h:22-26).  Attributes may appear in any order;
    missing ones keep their defaults."""
    mm = re.fullmatch(r'\s*Merl\(\s*"([^"]*)"\s*\)\s*', s)
    if mm:          # merl_data's string form, Merl("filename") (merl.h:60, :161-164)
        from .merl import Merl
        return Merl(mm.group(1))
    tok = _tokenize(s)
    m, i = _parse_model(tok, 0, s)
    if i != len(tok):
        raise ValueError(f"malformed BSDF string: {s!r}")
    return m


bsdf_import = fromString


def parse_model(s):
    """fromString through the library's own C-ABI parser (bbm_hip_parse_model_tree, the restatement of the
    reference's runtime fromString, bsdf_string_convert.h:52-85, that FFI callers use): the same models as
    fromString, built from the parser's preorder tree -- registry leaves (a fused runtime aggregate keeps its
    BBM_HIP_RUNTIME_AGGREGATE id), BBM_HIP_AGGREGATE_BSDF nodes as runtime AggregateModels."""
    lib = _lib.load()
    cap_nodes, cap_params = 256, 1 << 14
    ids, nk, npar = (ctypes.c_int * cap_nodes)(), (ctypes.c_int * cap_nodes)(), (ctypes.c_int * cap_nodes)()
    buf = np.zeros(cap_params, np.float32)
    k = _lib.check(lib.bbm_hip_parse_model_tree(s.encode(), ids, nk, buf.ctypes.data_as(ctypes.c_void_p), npar,
                                                 cap_nodes, cap_params))
    pos = [0, 0]            # next node, next parameter

    def build():
        i = pos[0]
        pos[0] += 1
        if ids[i] == _lib.AGGREGATE_BSDF:
            return AggregateModel(*[build() for _ in range(nk[i])], runtime=True)
        mid = ids[i]
        m = BsdfModel(lib.bbm_hip_model_name(mid & ~_lib.RUNTIME_AGGREGATE).decode())
        m.set_parameter_values(buf[pos[1]:pos[1] + npar[i]])
        pos[1] += npar[i]
        m.model_id = mid
        return m
    m = build()
    assert pos[0] == k
    return m


def _copy_model(m):
    """A copy of a model for an aggregate (aggregatemodel_base copies its children, aggregatemodel.h:34): same
    class, own parameter vector, and every other attribute shared -- a Merl child keeps the reference to the
    device table its parameters point to."""
    if isinstance(m, AggregateModel):
        return AggregateModel(*m._children, runtime=m.runtime)
    c = copy.copy(m)
    c._params = m._params.copy()
    return c


class AggregateModel:
    """aggregatemodel<MODELS...> (include/bsdfmodel/aggregatemodel.h:22-222) of any >= 2 models -- single models,
    Merl, fused aggregates, or composed aggregates again (aggregatemodel_base takes any bsdfmodel child, :22) --
    evaluated by composing the children's kernels (bbm_hip_aggregate_*, bbm_amd/csrc/composite.hip): eval /
    reflectance = the children's sum (right fold), pdf = their reflectance-weighted mixture, sample = the
    reference's child selection on xi0; a nested aggregate is one child with its own eval / pdf / sample /
    reflectance.  The published fits' form Aggregate(Lambertian, X) has fused kernels instead (Aggregate(...)
    picks them).  Parameters are the children's vectors in order (reflection order of the base classes).
    float32 tensors evaluate in floatRGB, float64 tensors in doubleRGB (every leaf needs doubleRGB kernels)."""

    def __init__(self, *children, runtime=False):
        if len(children) < 2:
            raise ValueError("an aggregate needs at least two child models")
        for c in children:
            if not isinstance(c, (BsdfModel, AggregateModel)):
                raise TypeError("aggregate children must be models (BsdfModel, Merl or AggregateModel)")
        self._children = [_copy_model(c) for c in children]
        self.name = aggregate_key([c.name for c in children])
        # runtime: the reference's aggregatebsdf (left folds, per-term pdf quotients, no sample unless the weights
        # sum to > eps; include/bbm/aggregatebsdf.h), what fromString builds; else aggregatemodel<...>
        self.runtime = bool(runtime)

    def children(self):
        return [_copy_model(c) for c in self._children]

    def parameter_values(self, flag=None):
        return np.concatenate([c.parameter_values(flag) for c in self._children])

    # the reference enumerates an aggregate's attributes child by child (bsdf_enumerate.h over the base classes)
    def parameter_attrs(self):
        return np.concatenate([c.parameter_attrs() for c in self._children])

    def parameter_indices(self, flag=0x0F):
        return np.nonzero(self.parameter_attrs() & np.uint32(flag))[0]

    def parameter_default_values(self):
        return np.concatenate([c.parameter_default_values() for c in self._children])

    def parameter_lower_bound(self):
        return np.concatenate([c.parameter_lower_bound() for c in self._children])

    def parameter_upper_bound(self):
        return np.concatenate([c.parameter_upper_bound() for c in self._children])

    def set_parameter_values(self, values):
        v = np.asarray(values, dtype=np.float32).reshape(-1)
        sizes = [c.parameter_values().size for c in self._children]
        if v.size != sum(sizes):
            raise ValueError(f"{self.name}: expected {sum(sizes)} parameters, got {v.size}")
        k = 0
        for c, n in zip(self._children, sizes):
            c.set_parameter_values(v[k:k + n])
            k += n

    def __str__(self):
        return "Aggregate(" + ", ".join(str(c) for c in self._children) + ")"

    __repr__ = __str__

    def has_f64(self):
        return all(c.has_f64() for c in self._children)

    def _desc(self, f64=False, params=None):
        """ctypes bbm_hip_child(_f64) tree: (array, count, keep-alive list of the arrays and parameter buffers it
        points to).  An aggregatemodel passes its children (count >= 2); a runtime aggregate passes its root node
        (count 1, BBM_HIP_AGGREGATE_BSDF), the only way to give the top level aggregatebsdf semantics.  Nested
        aggregates are AGGREGATE / AGGREGATE_BSDF nodes.  params: the flat parameter vector to use instead of the
        children's own (the leaves in preorder)."""
        keep = []
        kind = _lib.ChildF64 if f64 else _lib.Child
        flat = None if params is None else np.asarray(params).reshape(-1)
        off = [0]

        def leaf_params(c):
            if flat is None:
                return c._params
            k = c._params.size
            off[0] += k
            return flat[off[0] - k:off[0]]

        def node(a, c):
            if isinstance(c, AggregateModel):
                sub = build(c._children)
                a.model_id, a.params, a.nparams = (_lib.AGGREGATE_BSDF if c.runtime else _lib.AGGREGATE), None, 0
                a.children, a.nchildren = ctypes.cast(sub, ctypes.c_void_p), len(c._children)
            else:
                c._pptr()          # a Merl child checks its table's device here
                p = np.ascontiguousarray(leaf_params(c), dtype=np.float64 if f64 else np.float32)
                keep.append(p)
                a.model_id, a.params, a.nparams = c.model_id, p.ctypes.data, p.size
                a.children, a.nchildren = None, 0

        def build(kids):
            arr = (kind * len(kids))()
            keep.append(arr)
            for a, c in zip(arr, kids):
                node(a, c)
            return arr
        if self.runtime:
            root = (kind * 1)()
            keep.append(root)
            node(root[0], self)
            return root, 1, keep
        return build(self._children), len(self._children), keep

    @staticmethod
    def _no_varying(varying):
        if varying is not None:
            raise NotImplementedError("varying: per-lane parameters are not available for composed aggregates")

    def has_varying(self):
        return False

    def has_table(self):
        return False

    def eval_pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *,
                 rgb=None, pdf=None, stream=None, mode=3, varying=None, normal=None, cosine=False, tangent=None):
        """normal, cosine, tangent: BsdfModel.eval_pdf's, staged -- a tree has no fused kernel, so the directions go
        through to_local(normal, ., tangent=tangent) and the cosine is the z of to_local(normal, in_).  A tangent
        always goes to the frame calls: a tree's children may be anisotropic."""
        if _world_normal(normal, cosine, varying, in_, out, tangent) is not None:
            li = to_local(normal, in_, mask, stream=stream, tangent=tangent)
            r = self.eval_pdf(li, to_local(normal, out, mask, stream=stream, tangent=tangent), component, unit, mask, rgb=rgb, pdf=pdf,
                              stream=stream, mode=mode)
            return (*r, li[2]) if cosine else r
        self._no_varying(varying)
        torch = _torch()
        f64 = _is_f64(in_)
        dt = torch.float64 if f64 else torch.float32
        ix, iy, iz, n = _soa(in_, what="in", dtype=dt)
        ox, oy, oz, _ = _soa(out, n, what="out", dtype=dt)
        mptr, _keep = _mask_ptr(mask, n)
        dev = torch.device("cuda", torch.cuda.current_device())
        if mode & 1:
            rgb = torch.empty((3, n), dtype=dt, device=dev) if rgb is None else _out_rows(rgb, 3, n, dev, "rgb", dt)
        if mode & 2:
            pdf = torch.empty((n,), dtype=dt, device=dev) if pdf is None else _out_rows(pdf, 0, n, dev, "pdf", dt)
        _on_stream(stream, _keep, rgb, pdf)
        d, nd, _kd = self._desc(f64)
        fn = _lib.load().bbm_hip_aggregate_eval_pdf_f64 if f64 else _lib.load().bbm_hip_aggregate_eval_pdf
        _lib.check(fn(d, nd, ix, iy, iz, ox, oy, oz, mptr, n, int(component), int(unit),
                      rgb[0].data_ptr() if mode & 1 else None, rgb[1].data_ptr() if mode & 1 else None,
                      rgb[2].data_ptr() if mode & 1 else None, pdf.data_ptr() if mode & 2 else None,
                      _stream_ptr(stream)))
        return rgb, pdf

    eval = BsdfModel.eval
    pdf = BsdfModel.pdf

    def sample(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, stream=None, varying=None):
        self._no_varying(varying)
        torch = _torch()
        f64 = _is_f64(out)
        dt = torch.float64 if f64 else torch.float32
        ox, oy, oz, n = _soa(out, what="out", dtype=dt)
        x0, x1 = (xi if isinstance(xi, (tuple, list)) else (xi[0], xi[1]))
        for x in (x0, x1):
            if x.dtype != dt or not x.is_cuda or x.numel() != n or x.stride(0) != 1:
                raise TypeError(f"xi: expected {str(dt).replace('torch.', '')} CUDA rows with one entry per direction")
        mptr, _keep = _mask_ptr(mask, n)
        dev = x0.device
        d = torch.empty((3, n), dtype=dt, device=dev)
        p = torch.empty((n,), dtype=dt, device=dev)
        f = torch.empty((n,), dtype=torch.int32, device=dev)
        _on_stream(stream, _keep, d, p, f)
        desc, nd, _kd = self._desc(f64)
        fn = _lib.load().bbm_hip_aggregate_sample_f64 if f64 else _lib.load().bbm_hip_aggregate_sample
        _lib.check(fn(desc, nd, ox, oy, oz, x0.data_ptr(), x1.data_ptr(), mptr, n, int(component),
                      int(unit), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(), f.data_ptr(),
                      _stream_ptr(stream)))
        return BsdfSample(d, p, f)

    def sample_eval(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, value=True,
                    weight=True, stream=None, exact=None, normal=None, tangent=None):
        """BsdfModel.sample_eval for a composed or runtime tree -- staged: a tree has no fused kernel, so this runs
        the tree's own sample and eval_pdf on the GPU (two launches, the direction goes through memory) and forms
        the weight with torch float32 ops under the same rule (value * direction_z / pdf where pdf > epsilon, else
        0).  -> (BsdfSample, value or None, weight or None).  floatRGB only; a tree has no exact mode of its own, so
        exact must be None.  normal: world space, staged as well -- to_local(normal, out), the above, then
        to_global(normal, direction), both with tangent= where one is given."""
        torch = _torch()
        if exact is not None:
            raise NotImplementedError("sample_eval: composed aggregates follow the process-wide mode (exact=None)")
        if _frame_rows(normal, tangent, out) is not None:
            _sample_eval_inputs(out, xi)
            s, v, w = self.sample_eval(to_local(normal, out, mask, stream=stream, tangent=tangent), xi, component, unit,
                                       mask, value=value, weight=weight, stream=stream)
            return BsdfSample(to_global(normal, s.direction, mask, stream=stream, tangent=tangent), s.pdf, s.flag), v, w
        _sample_eval_inputs(out, xi)
        s = self.sample(out, xi, component, unit, mask, stream=stream)
        if not (value or weight):
            return s, None, None
        v = self.eval_pdf(s.direction, out, component, unit, mask, stream=stream, mode=1)[0]
        w = None
        if weight:
            run = torch.cuda.current_stream() if stream is None else stream
            with torch.cuda.stream(run):
                w = _weight(v, s.direction, s.pdf)
        return s, (v if value else None), w

    def reflectance(self, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, stream=None,
                    varying=None):
        self._no_varying(varying)
        torch = _torch()
        f64 = _is_f64(out)
        dt = torch.float64 if f64 else torch.float32
        ox, oy, oz, n = _soa(out, what="out", dtype=dt)
        mptr, _keep = _mask_ptr(mask, n)
        dev = (out[0] if isinstance(out, (tuple, list)) else out).device
        rgb = torch.empty((3, n), dtype=dt, device=dev)
        _on_stream(stream, _keep, rgb)
        desc, nd, _kd = self._desc(f64)
        fn = _lib.load().bbm_hip_aggregate_reflectance_f64 if f64 else _lib.load().bbm_hip_aggregate_reflectance
        _lib.check(fn(desc, nd, ox, oy, oz, mptr, n, int(component), int(unit), rgb[0].data_ptr(),
                      rgb[1].data_ptr(), rgb[2].data_ptr(), _stream_ptr(stream)))
        return rgb


def tree_desc(model, f64=False):
    """Any model as a bbm_hip_child(_f64) tree for the *_tree entry points (bbm_hip_loss_tree, bbm_hip_check_tree):
    (array, count, keep-alive list).  A single model (or fused aggregate, Merl) is one leaf node; an AggregateModel
    its children or its runtime root node (AggregateModel._desc)."""
    if isinstance(model, AggregateModel):
        return model._desc(f64)
    kind = _lib.ChildF64 if f64 else _lib.Child
    arr = (kind * 1)()
    p = model._pptr() if not f64 else None
    params = np.ascontiguousarray(model._params, dtype=np.float64) if f64 else model._params
    arr[0].model_id, arr[0].params, arr[0].nparams = model.model_id, params.ctypes.data, params.size
    arr[0].children, arr[0].nchildren = None, 0
    return arr, 1, [arr, params, p]


def Aggregate(*children, fused=True, runtime=False):
    """aggregate(models...) (aggregatemodel.h:232-233): the fused kernel for the published fits' form
    Aggregate(Lambertian, X) where one is registered (fused=False forces the composed path), otherwise an
    AggregateModel over the children's own kernels.

    Note: this mirrors the C++ template aggregate() (aggregatemodel<...>), NOT the reference's Python binding
    bbm.Aggregate (include/python/py_core.h:116-123), which builds the runtime aggregatebsdf of bsdf_ptrs.  The two
    differ in the pdf's rounding (inner product / sum here, per-term there) and in sampling (here a child is sampled
    even when the weights sum below eps).  Scripts ported from the reference's Python API get the binding's
    semantics with runtime=True, or with fromString("Aggregate(...)"), which returns runtime aggregates like
    bsdf_import does."""
    key = aggregate_key([c.name for c in children])
    if fused and key in AGGREGATES and all(isinstance(c, BsdfModel) for c in children):
        m = BsdfModel(key, *children)
        if runtime:
            m.model_id |= _lib.RUNTIME_AGGREGATE
        return m
    return AggregateModel(*children, runtime=runtime)


class MaterialTable:
    """M parameter sets of one model, evaluated in one launch with a material index per lane (bbm_hip_table_*,
    DESIGN.md §4.15): a wavefront renderer's material id per hit, the materials of one fits file over one direction
    set.  `params` is an (M, nparams) float32 array of raw parameter vectors (BsdfModel.parameter_values()); the
    library prepares and uploads them once, on `stream` (default: the current stream).  eval_pdf / eval / pdf /
    sample / reflectance take the arguments of the BsdfModel methods with `material=`, an int32 CUDA tensor of one
    index per lane, and return the same shapes; lane i gets exactly what the BsdfModel call returns for material
    material[i].  A negative or otherwise out-of-range index is a masked lane.  floatRGB only."""

    def __init__(self, model_name, params, *, runtime=False, stream=None):
        lib = _lib.load()
        self._handle = None
        if not isinstance(model_name, str):
            raise TypeError("MaterialTable: model_name must be a registry name (MaterialTable.from_models takes models)")
        mid = lib.bbm_hip_model_id(model_name.encode())
        if mid < 0:
            raise ValueError(f"unknown BSDF model: {model_name}")
        if runtime:
            mid |= _lib.RUNTIME_AGGREGATE
        p = np.asarray(params)
        if p.dtype == np.float64:
            raise TypeError("MaterialTable: material tables are floatRGB only (float32 parameters)")
        if p.dtype != np.float32:
            raise TypeError(f"MaterialTable: expected float32 parameters, got {p.dtype}")
        k = _lib.check(lib.bbm_hip_model_nparams(mid))
        if p.ndim != 2 or p.shape[0] < 1 or p.shape[1] != k:
            raise ValueError(f"MaterialTable: {model_name}: expected an (M, {k}) array with M >= 1, got {p.shape}")
        p = np.ascontiguousarray(p)
        handle = ctypes.c_void_p()
        # a row without table kernels is refused by the library before it looks at the stream: no GPU needed for that
        sptr = _stream_ptr(stream) if lib.bbm_hip_model_has_table(mid) == 1 else None
        _lib.check(lib.bbm_hip_table_create(mid, p.ctypes.data_as(ctypes.c_void_p), k, p.shape[0], sptr,
                                            ctypes.byref(handle)))
        self._handle = handle
        self.name = model_name
        self.model_id = mid
        self._size = int(p.shape[0])

    @classmethod
    def from_models(cls, models, *, stream=None):
        """A table of BsdfModels or model strings (fromString); all must be the same registry model."""
        ms = [fromString(m) if isinstance(m, str) else m for m in models]
        if not ms:
            raise ValueError("MaterialTable.from_models: no models")
        for m in ms:
            if isinstance(m, AggregateModel):
                raise NotImplementedError("MaterialTable: composed aggregates have no material tables (fused "
                                          "Aggregate(Lambertian, X) models do)")
            if not isinstance(m, BsdfModel):
                raise TypeError("MaterialTable.from_models: expected BsdfModels or model strings")
        if any(m.model_id != ms[0].model_id for m in ms):
            raise ValueError("MaterialTable.from_models: every model must be the same registry model, got " +
                             ", ".join(sorted({m.name + (" (runtime)" if m.runtime else "") for m in ms})))
        return cls(ms[0].name, np.stack([m.parameter_values() for m in ms]).astype(np.float32), runtime=ms[0].runtime,
                   stream=stream)

    def __len__(self):
        return self._size

    def close(self):
        """Release the table's device memory (waits for the device: launches already enqueued finish first)."""
        h, self._handle = self._handle, None
        if h is not None:
            _lib.load().bbm_hip_table_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def _live(self):
        if self._handle is None:
            raise ValueError("MaterialTable: the table is closed")
        return self._handle

    @staticmethod
    def _flags(exact):
        return 0 if exact is None else (_lib.CALL_EXACT if exact else _lib.CALL_DEFAULT)

    @staticmethod
    def _material(material, n, device):
        """The index tensor's pointer: int32, on the inputs' device, n elements with unit stride.  Its bits are read
        as uint32, so a negative index is out of range: a masked lane."""
        torch = _torch()
        if not isinstance(material, torch.Tensor) or material.dtype != torch.int32 or not material.is_cuda or \
                material.device != device:
            raise TypeError(f"material: expected an int32 CUDA tensor on {device}")
        if material.dim() != 1 or material.numel() != n:
            raise ValueError(f"material: expected {n} indices, got shape {tuple(material.shape)}")
        if n > 1 and material.stride(0) != 1:
            raise ValueError("material: indices must have unit stride")
        return material.data_ptr()

    def eval_pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material,
                 rgb=None, pdf=None, stream=None, mode=3, exact=None, normal=None, cosine=False, tangent=None):
        """normal, cosine, tangent: as BsdfModel.eval_pdf's (bbm_hip_eval_pdf_table_world and its _tangent form)."""
        nptr = _world_normal(normal, cosine, None, in_, out, tangent)
        if _is_f64(in_) or _is_f64(out):
            raise TypeError("MaterialTable: material tables are floatRGB only (float32 tensors)")
        h = self._live()
        ix, iy, iz, n = _soa(in_, what="in")
        ox, oy, oz, _ = _soa(out, n, what="out")
        dev = _device(in_)
        idx = self._material(material, n, dev)
        mptr, _keep = _mask_ptr(mask, n)
        rgb, pdf = _eval_pdf_outputs(mode, n, dev, rgb, pdf)
        _on_stream(stream, _keep, rgb, pdf, material)
        if nptr is not None:
            cos = _torch().empty((n,), dtype=_torch().float32, device=dev) if cosine else None
            _on_stream(stream, cos)
            _lib.check(_frame_fn("bbm_hip_eval_pdf_table_world", nptr)(
                h, self._flags(exact), idx, *nptr, ix, iy, iz, ox, oy, oz, mptr, n, int(component), int(unit),
                *_eval_pdf_ptrs(mode, rgb, pdf), None if cos is None else cos.data_ptr(), _stream_ptr(stream)))
            return (rgb, pdf, cos) if cosine else (rgb, pdf)
        _lib.check(_lib.load().bbm_hip_eval_pdf_table(
            h, self._flags(exact), idx, ix, iy, iz, ox, oy, oz, mptr, n, int(component), int(unit),
            *_eval_pdf_ptrs(mode, rgb, pdf), _stream_ptr(stream)))
        return rgb, pdf

    def eval(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=1, **kw), 0, kw.get("cosine", False))

    def pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=2, **kw), 1, kw.get("cosine", False))

    def sample(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material, stream=None,
               exact=None):
        torch = _torch()
        if _is_f64(out):
            raise TypeError("MaterialTable: material tables are floatRGB only (float32 tensors)")
        h = self._live()
        ox, oy, oz, n = _soa(out, what="out")
        x0, x1 = _xi_rows(xi, n, torch.float32)
        dev = x0.device
        idx = self._material(material, n, dev)
        mptr, _keep = _mask_ptr(mask, n)
        d, p, f = _sample_outputs(n, dev, torch.float32)
        _on_stream(stream, _keep, d, p, f, material)
        _lib.check(_lib.load().bbm_hip_sample_table(
            h, self._flags(exact), idx, ox, oy, oz, x0.data_ptr(), x1.data_ptr(), mptr, n, int(component), int(unit),
            d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(), f.data_ptr(), _stream_ptr(stream)))
        return BsdfSample(d, p, f)

    def sample_eval(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material,
                    value=True, weight=True, stream=None, exact=None, normal=None, tangent=None):
        """BsdfModel.sample_eval with a material per lane (bbm_hip_sample_eval_table): lane i gets what the table's
        sample followed by its eval_pdf at the sampled direction returns for material[i], and the weight.  normal,
        tangent: as BsdfModel.sample_eval's (bbm_hip_sample_eval_table_world and its _tangent form)."""
        nptr = _frame_rows(normal, tangent, out)
        ox, oy, oz, n, x0, x1 = _sample_eval_inputs(out, xi)
        h = self._live()
        dev = x0.device
        idx = self._material(material, n, dev)
        mptr, _keep = _mask_ptr(mask, n)
        outs = _sample_eval_outputs(n, dev, value, weight)
        _on_stream(stream, _keep, material, *outs)
        d, p, f, v, w = outs
        lib = _lib.load()
        fn, pre = ((lib.bbm_hip_sample_eval_table, ()) if nptr is None else
                   (_frame_fn("bbm_hip_sample_eval_table_world", nptr), nptr))
        _lib.check(fn(
            h, self._flags(exact), idx, *pre, ox, oy, oz, x0.data_ptr(), x1.data_ptr(), mptr, n, int(component), int(unit),
            d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), p.data_ptr(), f.data_ptr(), *_row_ptrs(v),
            *_row_ptrs(w), _stream_ptr(stream)))
        return BsdfSample(d, p, f), v, w

    def reflectance(self, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material, stream=None,
                    exact=None):
        torch = _torch()
        if _is_f64(out):
            raise TypeError("MaterialTable: material tables are floatRGB only (float32 tensors)")
        h = self._live()
        ox, oy, oz, n = _soa(out, what="out")
        dev = _device(out)
        idx = self._material(material, n, dev)
        mptr, _keep = _mask_ptr(mask, n)
        rgb = torch.empty((3, n), dtype=torch.float32, device=dev)
        _on_stream(stream, _keep, rgb, material)
        _lib.check(_lib.load().bbm_hip_reflectance_table(
            h, self._flags(exact), idx, ox, oy, oz, mptr, n, int(component), int(unit), rgb[0].data_ptr(),
            rgb[1].data_ptr(), rgb[2].data_ptr(), _stream_ptr(stream)))
        return rgb


def group_models(models):
    """MaterialSet.from_models' grouping, with no table made: BsdfModels or model strings of any rows ->
    (groups, material_ids).  groups: one (name, runtime, [models]) per (model_id, runtime) in order of first
    appearance; material_ids: int32, the global id of each input model in input order (table k's ids follow table
    k - 1's).  Rows without table kernels and composed aggregates are refused as MaterialTable refuses them."""
    ms = [fromString(m) if isinstance(m, str) else m for m in models]
    if not ms:
        raise ValueError("MaterialSet.from_models: no models")
    groups, where = [], {}
    for m in ms:
        if isinstance(m, AggregateModel):
            raise NotImplementedError("MaterialTable: composed aggregates have no material tables (fused "
                                      "Aggregate(Lambertian, X) models do)")
        if not isinstance(m, BsdfModel):
            raise TypeError("MaterialSet.from_models: expected BsdfModels or model strings")
        if not m.has_table():
            raise _lib.BackboneError(_lib.ERR_UNSUPPORTED, f"{m.name}: no material-table kernels")
        key = (m.model_id, m.runtime)
        if key not in where:
            where[key] = len(groups)
            groups.append((m.name, m.runtime, []))
        groups[where[key]][2].append(m)
    first = np.concatenate([[0], np.cumsum([len(g[2]) for g in groups])])
    seen = [0] * len(groups)
    ids = np.empty(len(ms), dtype=np.int32)
    for i, m in enumerate(ms):
        k = where[(m.model_id, m.runtime)]
        ids[i] = first[k] + seen[k]
        seen[k] += 1
    return groups, ids


class _DevicePtr:
    """Device memory of the library as a CUDA array, for torch.as_tensor."""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def _four_byte_rows(t, length, device, what):
    """A stream argument of MaterialPlan.gather / scatter: a CUDA tensor of a four-byte dtype on the plan's device,
    shaped (length,) or (k, length) with contiguous rows -> the device pointer of every row."""
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != 4 or t.is_complex():
        raise TypeError(f"{what}: expected a CUDA tensor of a four-byte dtype (float32, int32, uint32)")
    if t.device != device:
        raise TypeError(f"{what}: must live on {device}, got {t.device}")
    if t.dim() not in (1, 2) or t.shape[-1] != length:
        raise ValueError(f"{what}: expected shape ({length},) or (k, {length}), got {tuple(t.shape)}")
    if length > 1 and t.stride(-1) != 1:
        raise ValueError(f"{what}: rows must be contiguous")
    if t.dim() == 1:
        return [t.data_ptr()]
    return [t.data_ptr() + 4 * r * t.stride(0) for r in range(t.shape[0])]


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


class MaterialPlan:
    """The stable partition of one batch's lanes by table (bbm_hip_set_plan_*), made by
    MaterialSet.plan and passed as `plan=` to any number of calls over the same hits.  drop=True makes the compact plan
    (bbm_hip_set_plan_create_compact): a lane whose id is out of range is in no slot, and only the
    calls with order="plan" take it.  `capacity` is the number of sorted slots (segments[-1]), `compact` whether lanes
    were dropped.  gather / scatter carry any four-byte streams between lane order and slot order."""

    def __init__(self, mset, material, stream=None, *, drop=False):
        torch = _torch()
        self._handle = None
        if not isinstance(material, torch.Tensor) or material.dim() != 1:
            raise TypeError("material: expected a 1-D int32 CUDA tensor")
        n = material.numel()
        idx = MaterialTable._material(material, n, material.device)
        _on_stream(stream, material)
        handle = ctypes.c_void_p()
        lib = _lib.load()
        create = lib.bbm_hip_set_plan_create_compact if drop else lib.bbm_hip_set_plan_create
        _lib.check(create(mset._live(), idx, n, _stream_ptr(stream), ctypes.byref(handle)))
        self._handle = handle
        self.compact = bool(drop)
        self.set = mset
        self.device = material.device
        self.lanes = n
        seg = (ctypes.c_uint64 * (mset.rows + 1))()
        _lib.check(_lib.load().bbm_hip_set_plan_segments(handle, seg, mset.rows + 1))
        self.segments = [int(v) for v in seg]
        self.capacity = self.segments[-1]

    def _live(self):
        if self._handle is None:
            raise ValueError("MaterialPlan: the plan is closed")
        self.set._live()
        return self._handle

    def gather(self, *tensors, mask=None, stream=None):
        """Lane order -> slot order (bbm_hip_set_plan_gather).  Each tensor: a CUDA tensor of a four-byte dtype shaped
        (lanes,) or (k, lanes) with contiguous rows; -> tensors of shape (capacity,) or (k, capacity) of the same
        dtypes, in argument order: slot j holds lane order()[j]'s element, a padding slot 0.  mask: a uint8 / bool
        (lanes,) tensor, or True for "every lane live": the (capacity,) uint8 mask in slot order comes last, 0 in
        padding slots.  One tensor and no mask: that tensor alone, not a tuple."""
        torch = _torch()
        h = self._live()
        n, cap, dev = self.lanes, self.capacity, self.device
        src, outs = [], []
        for k, t in enumerate(tensors):
            src += _four_byte_rows(t, n, dev, f"gather: tensor {k}")
            outs.append(torch.empty(t.shape[:-1] + (cap,), dtype=t.dtype, device=dev))
        dst = [p for o in outs for p in _four_byte_rows(o, cap, dev, "gather: output")]
        mfrom = mto = keep = None
        if mask is not None and mask is not False:
            if mask is not True:
                mfrom, keep = _mask_ptr(mask, n)
            mto = torch.empty((cap,), dtype=torch.uint8, device=dev)
            outs.append(mto)
        _on_stream(stream, keep, *tensors, *outs)
        _lib.check(_lib.load().bbm_hip_set_plan_gather(
            h, _ptr_array(src), _ptr_array(dst), len(src), mfrom, None if mto is None else mto.data_ptr(), n,
            _stream_ptr(stream)))
        return outs[0] if len(outs) == 1 else tuple(outs)

    def scatter(self, *tensors, out=None, stream=None):
        """Slot order -> lane order (bbm_hip_set_plan_scatter), the inverse of gather: tensors of shape (capacity,) or
        (k, capacity) -> tensors of shape (lanes,) or (k, lanes).  Without out= the results start as zeros, so a lane
        a compact plan dropped reads 0; with out= (a tuple of tensors of the results' shapes and dtypes) such lanes
        keep what they held.  One tensor: that result alone, not a tuple."""
        torch = _torch()
        h = self._live()
        n, cap, dev = self.lanes, self.capacity, self.device
        if out is not None:
            out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
            if len(out) != len(tensors):
                raise ValueError(f"scatter: out= holds {len(out)} tensors for {len(tensors)} streams")
        src, dst, outs, keep = [], [], [], []
        for k, t in enumerate(tensors):
            rows = _four_byte_rows(t, cap, dev, f"scatter: tensor {k}")
            if any(p % 16 for p in rows):            # the slot-order side is read 16 bytes at a time
                t = t.clone(memory_format=torch.contiguous_format)
                rows = _four_byte_rows(t, cap, dev, f"scatter: tensor {k}")
            keep.append(t)
            src += rows
            shape = t.shape[:-1] + (n,)
            if out is None:
                o = torch.zeros(shape, dtype=torch.int32, device=dev).view(t.dtype)
            else:
                o = out[k]
                if not isinstance(o, torch.Tensor) or o.dtype != t.dtype or tuple(o.shape) != tuple(shape):
                    raise ValueError(f"scatter: out[{k}]: expected a {t.dtype} tensor of shape {tuple(shape)}")
            dst += _four_byte_rows(o, n, dev, f"scatter: out[{k}]")
            outs.append(o)
        _on_stream(stream, *keep, *outs)
        _lib.check(_lib.load().bbm_hip_set_plan_scatter(h, _ptr_array(src), _ptr_array(dst), len(src), n,
                                                        _stream_ptr(stream)))
        return outs[0] if len(outs) == 1 else tuple(outs)

    def order(self):
        """The source lane of every sorted slot: an int32 CUDA tensor of the plan's capacity, -1 in padding slots."""
        torch = _torch()
        h = self._live()
        cap = self.segments[-1]
        if cap == 0:
            return torch.empty((0,), dtype=torch.int32, device=self.device)
        ptr = _lib.load().bbm_hip_set_plan_order(h)
        with torch.cuda.device(self.device):
            return torch.as_tensor(_DevicePtr(ptr, cap), device=self.device).clone()

    def close(self):
        """Release the plan's device memory (waits for the device: calls already enqueued finish first)."""
        h, self._handle = self._handle, None
        if h is not None:
            _lib.load().bbm_hip_set_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


class MaterialSet:
    """Material tables of different models behind one global material id per lane (bbm_hip_set_*):
    table k owns the ids [offsets[k], offsets[k + 1]).  eval_pdf / eval / pdf / sample_eval take MaterialTable's
    arguments with `material=` (global ids, an int32 CUDA tensor) or `plan=` (a MaterialPlan of the same hits, made
    once by plan() and shared by several calls), and return the same shapes; lane i gets exactly what its table's call
    returns for it.  An id out of range is table 0's masked-index lane.  The set keeps its tables alive."""

    def __init__(self, tables):
        self._handle = None
        tables = list(tables)
        if not all(isinstance(t, MaterialTable) for t in tables):
            raise TypeError("MaterialSet: expected MaterialTables")
        arr = (ctypes.c_void_p * max(len(tables), 1))(*[t._live().value for t in tables])
        handle = ctypes.c_void_p()
        _lib.check(_lib.load().bbm_hip_set_create(arr, len(tables), ctypes.byref(handle)))
        self._handle = handle
        self.tables = tables
        self.material_ids = None
        lib = _lib.load()
        self.rows = int(lib.bbm_hip_set_rows(handle))
        self.offsets = [int(lib.bbm_hip_set_offset(handle, k)) for k in range(self.rows + 1)]

    @classmethod
    def from_models(cls, models, *, stream=None):
        """A set of BsdfModels or model strings of different rows: one MaterialTable per (model, runtime) group in
        order of first appearance; `material_ids` holds each input model's global id, in input order."""
        groups, ids = group_models(models)
        s = cls([MaterialTable.from_models(ms, stream=stream) for _, _, ms in groups])
        s.material_ids = ids
        return s

    def __len__(self):
        return self.offsets[-1]

    def close(self):
        """Release the set (not its tables, which other sets may share)."""
        h, self._handle = self._handle, None
        if h is not None:
            _lib.load().bbm_hip_set_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def _live(self):
        if self._handle is None:
            raise ValueError("MaterialSet: the set is closed")
        return self._handle

    def plan(self, material, stream=None, *, drop=False):
        """Partition one batch's lanes by table: a MaterialPlan for `plan=`.  Waits for the stream once.  drop=True:
        the lanes whose id is out of range (terminated paths) are left out of the plan (MaterialPlan)."""
        return MaterialPlan(self, material, stream, drop=drop)

    @staticmethod
    def _sorted(order, material, plan):
        """order= of the calls: "lanes" (False) or "plan" (True), which needs plan= and excludes material=.  A compact
        plan has no lane-order call: its dropped lanes would get no output."""
        if order not in ("lanes", "plan"):
            raise ValueError(f'order: expected "lanes" or "plan", got {order!r}')
        if order == "plan":
            if plan is None or material is not None:
                raise ValueError('order="plan" needs plan= (and no material=): the streams are in that plan\'s slot order')
            return True
        if isinstance(plan, MaterialPlan) and plan.compact:
            raise ValueError('a compact plan (drop=True) leaves lanes out: call it with order="plan"')
        return False

    def _planned(self, material, plan, stream, n, device):
        """(the plan to use, whether it is this call's own)."""
        if (material is None) == (plan is None):
            raise ValueError("MaterialSet: give material= (global ids) or plan= (a MaterialPlan), not both")
        self._live()
        if plan is None:
            MaterialTable._material(material, n, device)
            return MaterialPlan(self, material, stream), True
        if not isinstance(plan, MaterialPlan) or plan.set is not self:
            raise ValueError("plan: expected a MaterialPlan made by this set")
        plan._live()
        return plan, False

    def eval_pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material=None,
                 plan=None, rgb=None, pdf=None, stream=None, mode=3, exact=None, normal=None, cosine=False,
                 tangent=None, order="lanes"):
        """tangent (with normal=): read by the rows whose model is anisotropic (bbm_hip_set_eval_pdf_tangent).
        order="plan" (with plan=): every input, mask, normal, tangent, rgb= and pdf= is in the plan's slot order and of
        length plan.capacity (MaterialPlan.gather), and so are the results: nothing is gathered or scattered
        (bbm_hip_set_eval_pdf_sorted)."""
        nptr = _world_normal(normal, cosine, None, in_, out, tangent)
        if _is_f64(in_) or _is_f64(out):
            raise TypeError("MaterialSet: material sets are floatRGB only (float32 tensors)")
        in_plan_order = self._sorted(order, material, plan)
        ix, iy, iz, n = _soa(in_, what="in")
        ox, oy, oz, _ = _soa(out, n, what="out")
        dev = _device(in_)
        mptr, _keep = _mask_ptr(mask, n)
        rgb, pdf = _eval_pdf_outputs(mode, n, dev, rgb, pdf)
        cos = _torch().empty((n,), dtype=_torch().float32, device=dev) if cosine else None
        _on_stream(stream, _keep, rgb, pdf, cos)
        p, own = self._planned(material, plan, stream, n, dev)
        try:
            fn, frame = ((_lib.load().bbm_hip_set_eval_pdf_sorted, _frame6(nptr)) if in_plan_order else
                         (_frame_fn("bbm_hip_set_eval_pdf", nptr), nptr or (None, None, None)))
            _lib.check(fn(
                p._live(), MaterialTable._flags(exact), *frame, ix, iy, iz, ox, oy, oz, mptr, n,
                int(component), int(unit), *_eval_pdf_ptrs(mode, rgb, pdf), None if cos is None else cos.data_ptr(),
                _stream_ptr(stream)))
        finally:
            if own:
                p.close()
        return (rgb, pdf, cos) if cosine else (rgb, pdf)

    def eval(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=1, **kw), 0, kw.get("cosine", False))

    def pdf(self, in_, out, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, **kw):
        return _with_cosine(self.eval_pdf(in_, out, component, unit, mask, mode=2, **kw), 1, kw.get("cosine", False))

    def sample_eval(self, out, xi, component=bsdf_flag.All, unit=unit_t.Radiance, mask=None, *, material=None,
                    plan=None, value=True, weight=True, stream=None, exact=None, normal=None, tangent=None,
                    order="lanes"):
        """order="plan": as eval_pdf's (bbm_hip_set_sample_eval_sorted)."""
        nptr = _frame_rows(normal, tangent, out)
        in_plan_order = self._sorted(order, material, plan)
        ox, oy, oz, n, x0, x1 = _sample_eval_inputs(out, xi)
        dev = x0.device
        mptr, _keep = _mask_ptr(mask, n)
        outs = _sample_eval_outputs(n, dev, value, weight)
        _on_stream(stream, _keep, *outs)
        d, p_, f, v, w = outs
        p, own = self._planned(material, plan, stream, n, dev)
        try:
            fn, frame = ((_lib.load().bbm_hip_set_sample_eval_sorted, _frame6(nptr)) if in_plan_order else
                         (_frame_fn("bbm_hip_set_sample_eval", nptr), nptr or (None, None, None)))
            _lib.check(fn(
                p._live(), MaterialTable._flags(exact), *frame, ox, oy, oz, x0.data_ptr(),
                x1.data_ptr(), mptr, n, int(component), int(unit), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                p_.data_ptr(), f.data_ptr(), *_row_ptrs(v), *_row_ptrs(w), _stream_ptr(stream)))
        finally:
            if own:
                p.close()
        return BsdfSample(d, p_, f), v, w


def _make_ctor(name):
    def ctor(*args, **kwargs):
        return BsdfModel(name, *args, **kwargs)
    ctor.__name__ = name
    if name in ATTRIBUTES:
        ctor.__doc__ = f"Constructs: {name}({', '.join(a for a, _ in ATTRIBUTES[name])}) -- {nparams(name)} parameters"
    return ctor


def scratch_trim():
    """Return the library's idle device scratch (per-launch temporaries of composed aggregates and tabulated
    samplers) to the device (bbm_hip_scratch_trim); returns the bytes freed."""
    return int(_lib.load().bbm_hip_scratch_trim())


def scratch_trim_captured():
    """Free the scratch blocks that HIP-graph captures of library calls hold (bbm_hip_scratch_trim_captured): only
    once every such graph is destroyed.  Returns the bytes freed."""
    return int(_lib.load().bbm_hip_scratch_trim_captured())


def scratch_bytes():
    """Device bytes the library's scratch pool currently holds (bbm_hip_scratch_bytes)."""
    return int(_lib.load().bbm_hip_scratch_bytes())


def set_exact_subnormals(on):
    """Exact-subnormal mode of the Beckmann microfacet models' eval / pdf kernels (bbm_hip_set_exact_subnormals,
    process-wide): on, the quotients a subnormal intermediate can reach round on the subnormal grid as the
    reference's IEEE divisions do, and CookTorrance & co. return the reference's floats bit for bit (+3.6-4.3 % kernel
    time on the headline); off (default), outputs below ~1e-30 may differ in the last bit.  Returns the previous
    setting."""
    return bool(_lib.load().bbm_hip_set_exact_subnormals(1 if on else 0))


def fill_directions(seed, stream_id, offset, n, mode=0, out=None, stream=None):
    """Counter-based synthetic directions (bbm_hip_fill_directions) -> (3, n) float32 CUDA tensor."""
    torch = _torch()
    if out is None:
        out = torch.empty((3, n), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    lib = _lib.load()
    _lib.check(lib.bbm_hip_fill_directions(seed, stream_id, offset, n, mode, out[0].data_ptr(), out[1].data_ptr(),
                                           out[2].data_ptr(), _stream_ptr(stream)))
    return out
