"""PFM images, byte-compatible with the reference's io::exportPFM / io::importPFM (include/io/pfm.h).

An image here is (3, H, W) -- the layout bbm_amd.render and bbm_amd.plot return -- with row y = 0 first; the file
stores rows bottom-up (y = H - 1 first), three little-endian floats per pixel, after the header
``PF\\n{w} {h}\\n-1.000000\\n``.  import_pfm also reads one-channel (``Pf``) and big-endian (positive scale) files.
"""
import re

import numpy as np


def _to_numpy(image):
    if hasattr(image, "detach"):          # a torch tensor, CUDA or not
        image = image.detach().cpu().numpy()
    return np.asarray(image)


def export_pfm(filename, image, channels=(0, 1, 2)):
    """exportPFM (pfm.h:34-76): write `image` ((C, H, W), or (H, W) for one channel) as a 3-channel little-endian PFM.
    channels: which image channel goes to each of the file's three; -1 or one the image lacks writes 0."""
    img = _to_numpy(image)
    if img.ndim == 2:
        img = img[None]
    if img.ndim != 3:
        raise ValueError(f"export_pfm: expected a (C, H, W) image, got shape {img.shape}")
    c, h, w = img.shape
    if w == 0 or h == 0:
        raise RuntimeError("io::exportPFM: No data in bitmap")
    if len(channels) != 3:
        raise ValueError("export_pfm: channels must name three channels")
    buf = np.zeros((h, w, 3), dtype="<f4")
    for k, ch in enumerate(channels):
        if 0 <= int(ch) < c:
            buf[:, :, k] = img[int(ch)][::-1]
    with open(filename, "wb") as f:
        f.write(b"PF\n" + f"{w} {h}\n".encode() + b"-1.000000\n")
        f.write(buf.tobytes())


def import_pfm(filename):
    """importPFM (pfm.h:91-155) -> (3, H, W) float32, row y = 0 first.  A one-channel file ('Pf') fills channel 0
    (the others stay 0, as a fresh bitmap's do); a positive scale line means big-endian data."""
    with open(filename, "rb") as f:
        data = f.read()
    if len(data) < 3 or data[0:1] != b"P":
        raise RuntimeError("io::importPFM: Not a recognized PFM format")
    nch = 1 if data[1:2] == b"f" else 3
    pos = 3

    def skip_comment(pos):
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
        return pos

    def token(pos):
        m = re.compile(rb"\s*(\S+)").match(data, pos)
        if not m:
            raise RuntimeError("io::importPFM: truncated header")
        return m.group(1), m.end()
    pos = skip_comment(pos)
    w, pos = token(pos)
    h, pos = token(pos)
    pos = skip_comment(pos + 1 if data[pos:pos + 1] == b"\n" and data[pos + 1:pos + 2] == b"#" else pos)
    scale, pos = token(pos)
    w, h, big = int(w), int(h), float(scale) > 0
    pos += 1                              # the single whitespace byte that ends the header
    n = w * h * nch
    raw = np.frombuffer(data, dtype=">f4" if big else "<f4", count=n, offset=pos)
    out = np.zeros((3, h, w), dtype=np.float32)
    out[:nch] = raw.reshape(h, w, nch)[::-1].transpose(2, 0, 1)
    return out
