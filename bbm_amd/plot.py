"""plotBsdf on the GPU -- the reference's bin/plotBsdf.cpp: a (phi, theta) slice of a BSDF's eval, pdf or sample
histogram for one view direction, as an image (bbm_hip_plot).

    python -m bbm_amd.plot bsdfmodel="GGX(roughness=0.3)" filename=slice.pfm plot=eval samples=16 view=[0.3,-0.2,0.9]

Options as in the reference (`key=value`, a bare key meaning true): bsdfmodel, filename, width, height, view, samples,
scale, maskZero, plot=<eval|pdf|sample>.

Random numbers: the reference draws from one std::mt19937; here draw g = (y * width + x) * samples + s (eval / pdf),
or the g-th sample (sample), comes from the library's counter-based generator on `seed` (plot_draws returns the same
numbers), or from the caller's own `xi`, a (2, width * height * samples) tensor in that order.

A single model or a fused aggregate runs the fused kernels; any other model (composed aggregates, runtime trees) the
staged path over its own eval / pdf / sample -- the same image bit for bit where both exist.
"""
import sys

import numpy as np

from . import _lib
from .backbone import AggregateModel, BsdfModel, _on_stream, _stream_ptr, _torch, fromString
from .check import DEFAULT_SEED, parse_options
from .render import _vec3, parse_vec3

KINDS = {"eval": 0, "pdf": 1, "sample": 2}
USAGE = ("[bsdfmodel=<bsdf string>] [filename=<name>] [width=512] [height=256] [view=[0,0,1]] [samples=1] [scale=1] "
         "[maskZero] [plot=<eval|pdf|sample>]")
KEYS = ("bsdfmodel", "filename", "width", "height", "view", "samples", "scale", "maskZero", "plot")


def plot_draws(seed, offset, n, stream=None):
    """The uniforms plot() uses for draws offset .. offset + n - 1 of `seed` -> (2, n) float32 CUDA tensor."""
    torch = _torch()
    u = torch.empty((2, int(n)), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    _on_stream(stream, u)
    _lib.check(_lib.load().bbm_hip_plot_draws(int(seed), int(offset), int(n), u[0].data_ptr(), u[1].data_ptr(),
                                              _stream_ptr(stream)))
    return u


def plot_directions(width, height, samples=1, xi=None, seed=DEFAULT_SEED, stream=None):
    """The light direction of every draw of plot eval / pdf -> (3, width * height * samples) float32 CUDA tensor."""
    torch = _torch()
    n = int(width) * int(height) * int(samples)
    d = torch.empty((3, max(n, 0)), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    x0, x1 = _xi_ptrs(xi, n)
    _on_stream(stream, d)
    _lib.check(_lib.load().bbm_hip_plot_dirs(int(width), int(height), int(samples), x0, x1, int(seed), d[0].data_ptr(),
                                             d[1].data_ptr(), d[2].data_ptr(), _stream_ptr(stream)))
    return d


def _xi_ptrs(xi, n):
    if xi is None:
        return None, None
    torch = _torch()
    if not isinstance(xi, torch.Tensor) or xi.dtype != torch.float32 or not xi.is_cuda or tuple(xi.shape) != (2, n) \
            or xi.stride(1) != 1:
        raise TypeError(f"xi: expected a (2, {n}) float32 CUDA tensor with contiguous rows")
    return xi[0].data_ptr(), xi[1].data_ptr()


def plot(model, kind, width=512, height=256, view=(0, 0, 1), samples=1, scale=1.0, maskZero=False, *, xi=None,
         seed=DEFAULT_SEED, return_counts=False, exact=None, stream=None):
    """plotBsdf's image of `model` -> (3, H, W) float32 CUDA tensor, row y = 0 (theta = 0) first.  kind: 'eval', 'pdf'
    or 'sample'.  return_counts ('sample' only): also the (H, W) int64 histogram the image is replayed from.
    exact: as BsdfModel.eval_pdf (fused path only)."""
    if kind not in KINDS:
        raise ValueError(f"unknown plotting command '{kind}'.")
    torch = _torch()
    lib = _lib.load()
    width, height, samples = int(width), int(height), int(samples)
    dev = torch.device("cuda", torch.cuda.current_device())
    npix = max(width * height, 0)
    n = npix * max(samples, 0)
    vvec = _vec3(view, "view")
    x0, x1 = _xi_ptrs(xi, n)
    img = torch.empty((3, max(height, 0), max(width, 0)), dtype=torch.float32, device=dev)
    counts = torch.empty((max(height, 0), max(width, 0)), dtype=torch.int64, device=dev) if kind == "sample" else None
    _on_stream(stream, img, counts)
    s = _stream_ptr(stream)
    k = KINDS[kind]
    if not isinstance(model, AggregateModel):
        if not isinstance(model, BsdfModel):
            raise TypeError("plot: model must be a BsdfModel or an AggregateModel")
        _lib.check(lib.bbm_hip_plot(model._call_id(exact), model._pptr(), model._params.size, k, width, height, vvec,
                                    samples, float(scale), int(bool(maskZero)), x0, x1, int(seed), img.data_ptr(),
                                    None if counts is None else counts.data_ptr(), s))
    else:
        if npix == 0 or samples <= 0:      # the library's argument errors, before anything is allocated per draw
            _lib.check(lib.bbm_hip_plot_dirs(width, height, samples, x0, x1, int(seed), None, None, None, s))
        v = np.asarray(view, dtype=np.float32).reshape(3)
        v = v * (np.float32(1) / np.sqrt(((np.float32(0) + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2], dtype=np.float32))
        if not np.all(np.isfinite(v)):
            raise _lib.BackboneError(_lib.ERR_INVALID_ARG, "view must be a finite non-zero vector")
        vd = torch.from_numpy(np.repeat(v.astype(np.float32)[:, None], n, axis=1)).to(dev)
        _on_stream(stream, vd)
        if kind == "sample":
            u = xi if xi is not None else plot_draws(seed, 0, n, stream)
            smp = model.sample(vd, u, stream=stream)
            _lib.check(lib.bbm_hip_plot_bin(width, height, n, smp.direction[0].data_ptr(), smp.direction[1].data_ptr(),
                                            smp.direction[2].data_ptr(), smp.pdf.data_ptr(), int(bool(maskZero)),
                                            counts.data_ptr(), s))
            _lib.check(lib.bbm_hip_plot_counts_image(counts.data_ptr(), width, height, samples, float(scale),
                                                     img.data_ptr(), s))
        else:
            ld = plot_directions(width, height, samples, xi, seed, stream)
            if kind == "eval":
                val = model.eval(ld, vd, stream=stream)
                r, g, b = val[0].data_ptr(), val[1].data_ptr(), val[2].data_ptr()
            else:
                val = model.pdf(ld, vd, stream=stream)
                r, g, b = val.data_ptr(), None, None
            _lib.check(lib.bbm_hip_plot_accumulate(k, width, height, samples, float(scale), x0, x1, int(seed), r, g, b,
                                                   img.data_ptr(), s))
    if return_counts:
        return img, counts
    return img


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        print(f"Usage: python -m bbm_amd.plot {USAGE}")
        return -1
    opt = parse_options(argv)
    invalid = [k for k in opt if k not in KEYS]
    if invalid:
        print(f"ERROR: invalid keywords: {invalid}.")
        return -1
    filename = opt.get("filename", "")
    width, height = int(opt.get("width", 512)), int(opt.get("height", 256))
    samples = int(opt.get("samples", 1))
    view = np.asarray(parse_vec3(opt["view"]) if "view" in opt else [0, 0, 1], dtype=np.float32)
    kind = opt.get("plot", "")
    scale = float(opt.get("scale", 1.0))
    mask_zero = opt.get("maskZero", "false").lower() in ("1", "true", "yes", "on")
    if kind not in KINDS:
        print(f"ERROR: unknown plotting command '{kind}'.")
        return -1
    if filename == "":
        print("ERROR: expected an output filename.")
        return -1
    bsdf = fromString(opt["bsdfmodel"]) if opt.get("bsdfmodel") else BsdfModel("Lambertian")
    with np.errstate(all="ignore"):
        shown = view * (np.float32(1) / np.sqrt(np.dot(view, view), dtype=np.float32))
    line = (f"Plotting '{kind}' to file '{filename}' with parameters: {bsdf} from "
            f"[{', '.join(f'{float(x):g}' for x in shown)}] at: {width} x {height} resolution")
    if mask_zero and kind == "sample":
        line += " => Masking samples with zero PDF"
    print(line + ".", flush=True)
    from .pfm import export_pfm
    export_pfm(filename, plot(bsdf, kind, width, height, view, samples, scale, mask_zero))
    return 0


if __name__ == "__main__":
    sys.exit(main())
