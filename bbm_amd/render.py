"""renderSphere on the GPU -- the reference's bin/renderSphere.cpp: a sphere lit by one directional light, every
pixel's shading frame, local directions, BSDF evaluation and cosine in one kernel (bbm_hip_render_sphere).

    python -m bbm_amd.render bsdfmodel="CookTorrance(roughness=0.3)" filename=sphere.pfm light=[1,-0.5,-1]

Options as in the reference (`key=value`, include/util/option.h): bsdfmodel, filename, light, width, height.
A single model or a fused aggregate runs the fused kernel; any other model (composed aggregates, runtime trees) runs
the staged path -- the same directions from bbm_hip_render_sphere_dirs, the model's own eval with the shaded mask,
and bbm_hip_render_shade -- which gives the same image bit for bit where both exist.
"""
import ctypes
import sys

import numpy as np

from . import _lib
from .backbone import AggregateModel, BsdfModel, _on_stream, _stream_ptr, _torch, fromString
from .check import parse_options

USAGE = "[bsdfmodel=<bsdf string>] [filename=<name>] [light=[0,0,1]] [width=512] [height=512]"
KEYS = ("bsdfmodel", "filename", "width", "height", "light")


def _vec3(v, what):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size != 3:
        raise ValueError(f"{what}: expected three components, got {a.size}")
    return (ctypes.c_float * 3)(*[float(x) for x in a])


def parse_vec3(s):
    """A Vec3d option: `[x,y,z]` or `x,y,z`."""
    return [float(t) for t in s.strip().lstrip("[").rstrip("]").split(",")]


def render_sphere(model, width=512, height=512, light=(0, 0, -1), *, return_dirs=False, exact=None, stream=None):
    """renderSphere's image of `model` (anything fromString, BsdfModel or Aggregate produces) -> (3, H, W) float32 CUDA
    tensor, row y = 0 first.  light: the light's direction of travel, any length (normalised as the tool does).
    return_dirs: also each pixel's local `in` and `out` ((3, H, W) each) and the shaded mask ((H, W) bool).
    exact: as BsdfModel.eval_pdf (fused path only)."""
    torch = _torch()
    lib = _lib.load()
    width, height = int(width), int(height)
    dev = torch.device("cuda", torch.cuda.current_device())
    npix = max(width * height, 0)
    lvec = _vec3(light, "light")
    staged = isinstance(model, AggregateModel)
    img = torch.empty((3, max(height, 0), max(width, 0)), dtype=torch.float32, device=dev)
    din = dout = mask = None
    if return_dirs or staged:
        din = torch.empty((3, npix), dtype=torch.float32, device=dev)
        dout = torch.empty((3, npix), dtype=torch.float32, device=dev)
        mask = torch.empty((npix,), dtype=torch.uint8, device=dev)
    _on_stream(stream, img, din, dout, mask)
    s = _stream_ptr(stream)

    def ptrs(t):
        return (None, None, None) if t is None else (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    if staged:
        _lib.check(lib.bbm_hip_render_sphere_dirs(width, height, lvec, *ptrs(din), *ptrs(dout), mask.data_ptr(), s))
        rgb = model.eval(din, dout, mask=mask, stream=stream)
        _lib.check(lib.bbm_hip_render_shade(npix, rgb[0].data_ptr(), rgb[1].data_ptr(), rgb[2].data_ptr(),
                                            din[2].data_ptr(), mask.data_ptr(), img.data_ptr(), s))
    else:
        if not isinstance(model, BsdfModel):
            raise TypeError("render_sphere: model must be a BsdfModel or an AggregateModel")
        _lib.check(lib.bbm_hip_render_sphere(model._call_id(exact), model._pptr(), model._params.size, width, height,
                                             lvec, img.data_ptr(), *ptrs(din), *ptrs(dout),
                                             None if mask is None else mask.data_ptr(), s))
    if return_dirs:
        # the mask's bytes are 0 / 1: reinterpreted, not converted (a conversion would run on the current stream)
        return img, din.view(3, height, width), dout.view(3, height, width), mask.view(height, width).view(torch.bool)
    return img


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        print(f"Usage: python -m bbm_amd.render {USAGE}")
        return -1
    opt = parse_options(argv)
    invalid = [k for k in opt if k not in KEYS]
    if invalid:
        print(f"ERROR: invalid keywords: {invalid}.")
        return -1
    filename = opt.get("filename", "")
    width, height = int(opt.get("width", 512)), int(opt.get("height", 512))
    light = np.asarray(parse_vec3(opt["light"]) if "light" in opt else [0, 0, -1], dtype=np.float32)
    if filename == "":
        print("ERROR: expected an output filename.")
        return -1
    bsdf = fromString(opt["bsdfmodel"]) if opt.get("bsdfmodel") else BsdfModel("Lambertian")
    with np.errstate(all="ignore"):
        shown = light * (np.float32(1) / np.sqrt(np.dot(light, light), dtype=np.float32))
    print(f"Rendering with parameters: {bsdf} to file '{filename}' with camera direction [0,0,-1] lit with a directional "
          f"light with direction: [{', '.join(f'{float(x):g}' for x in shown)}] at: {width} x {height}", flush=True)
    from .pfm import export_pfm
    export_pfm(filename, render_sphere(bsdf, width, height, light))
    return 0


if __name__ == "__main__":
    sys.exit(main())
