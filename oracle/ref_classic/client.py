"""Python side of oracle/_ref/ref_classic (built by build_ref.py): one child process per call, raw arrays through two temporary files.
Test and fixture-generation infrastructure only; nothing here runs on a GPU machine."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from . import build_ref

_CODES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2}
_DTYPES = {v: k for k, v in _CODES.items()}


class RefError(RuntimeError):
    pass


def binary(sanitized=False):
    return os.path.join(build_ref.OUT, "ref_classic_san" if sanitized else "ref_classic")


def usable(sanitized=False):
    """the harness exists AND the checkout it was cut from is present (a leftover build without its source is not trusted)"""
    return os.path.isfile(binary(sanitized)) and build_ref.available()


def _write(path, arrays):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(arrays)))
        for a in arrays:
            a = np.ascontiguousarray(a)
            f.write(struct.pack("<iq", _CODES[a.dtype], a.size))
            f.write(a.tobytes())


def _read(path):
    with open(path, "rb") as f:
        raw = f.read()
    (count,), pos, out = struct.unpack_from("<i", raw, 0), 4, []
    for _ in range(count):
        code, n = struct.unpack_from("<iq", raw, pos)
        pos += 12
        dt = _DTYPES[code]
        out.append(np.frombuffer(raw, dt, n, pos).copy())
        pos += n * dt.itemsize
    return out


def run(op, arrays, sanitized=False, timeout=600):
    exe = binary(sanitized)
    if not os.path.isfile(exe):
        raise RefError(f"{exe} is not built (python oracle/ref_classic/build_ref.py)")
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        _write(fin, arrays)
        r = subprocess.run([exe, op, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        if r.returncode != 0:
            raise RefError(f"ref_classic {op} ended with {r.returncode}: {r.stderr.decode(errors='replace')[-2000:]}")
        return _read(fout)


def _f(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def stereo(img_l, img_r, k_l, oct_l, k_r, oct_r, d_l, d_r, mb, mbf, nlevels=1, scale_factor=1.2, sanitized=False):
    """Frame::ComputeStereoMatches on level-0 images; returns (mvuRight [N], mvDepth [N])"""
    il, ir = np.ascontiguousarray(img_l, np.uint8), np.ascontiguousarray(img_r, np.uint8)
    H, W = il.shape
    kl, kr = _f(k_l, (-1, 2)), _f(k_r, (-1, 2))
    pi = np.array([H, W, nlevels, len(kl), len(kr)], np.int32)
    pf = np.array([mb, mbf, scale_factor], np.float32)
    u, z = run("stereo", [pi, pf, il, ir, kl, np.ascontiguousarray(oct_l, np.int32), kr, np.ascontiguousarray(oct_r, np.int32),
                          _f(d_l, (-1, 256)), _f(d_r, (-1, 256))], sanitized)
    return u, z


def geometry(H, W, nlevels, scale_factor, nfeatures=1000, sanitized=False):
    """SPextractor's constructor and ComputePyramid's level sizes: dict scale, inv, level_w, level_h, fpl"""
    s, inv, lw, lh, fpl = run("geometry", [np.array([H, W, nlevels, nfeatures], np.int32), np.array([scale_factor], np.float32)], sanitized)
    return {"scale": s, "inv": inv, "level_w": lw, "level_h": lh, "fpl": fpl}


def distance(a, b, sanitized=False):
    a, b = _f(a, (-1, 256)), _f(b, (-1, 256))
    return run("distance", [a, b], sanitized)[0].reshape(len(a), len(b))


def distinctive(desc, offsets, sanitized=False):
    return run("distinctive", [_f(desc, (-1, 256)), np.ascontiguousarray(offsets, np.int32)], sanitized)[0]


def normalize_keypoints(kpts, h, w, sanitized=False):
    k = _f(kpts, (-1, 2))
    return run("normkp", [k, np.array([h, w], np.int32)], sanitized)[0].reshape(-1, 2)


def binarize(desc, sanitized=False):
    d = _f(desc, (-1, 256))
    return run("binarize", [d], sanitized)[0].reshape(-1, 256)
