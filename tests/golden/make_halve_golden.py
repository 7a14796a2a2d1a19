"""Writes tests/golden/halve_reference.npz: what the reference's mve::image::rescale_half_size<uint8_t> makes of every
image of tests/view_cases.halve_images(), as bytes in the output's shape, every step of the chains of
view_cases.HALVE_CHAINS (the reference halving its own last result), and under "refused" whether it threw on
view_cases.REFUSED_SHAPE.

The reference is compiled here from its own headers (REF, as in make_sift_golden.py) with the driver beside this file
into a temporary directory; nothing of it enters the tree.  The script then holds the numpy restatement
(view_cases.halve) against what it wrote.

    python tests/golden/make_halve_golden.py
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import view_cases as vc  # noqa: E402
from make_sift_golden import MVE  # noqa: E402


def compile_driver(tmp):
    exe = os.path.join(tmp, "halve_golden_driver")
    subprocess.check_call(["g++", "-O2", "-msse3", "-std=c++11", "-w", "-DMVE_NO_PNG_SUPPORT", "-DMVE_NO_JPEG_SUPPORT",
                           "-DMVE_NO_TIFF_SUPPORT", "-I" + MVE, "-o", exe, os.path.join(HERE, "halve_golden_driver.cc")])
    return exe


def run_reference(exe, tmp, name, img):
    """The halved image, or None where the reference refuses."""
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    raw, out = os.path.join(tmp, name + ".raw"), os.path.join(tmp, name + ".out")
    np.ascontiguousarray(img).tofile(raw)
    rc = subprocess.call([exe, raw, str(w), str(h), str(c), out], stderr=subprocess.DEVNULL)
    if rc == 3:
        return None
    assert rc == 0, (name, rc)
    ow, oh = (w + 1) >> 1, (h + 1) >> 1
    return np.fromfile(out, np.uint8).reshape((oh, ow) if c == 1 else (oh, ow, c))


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        for name, img in vc.halve_images().items():
            out[name] = run_reference(exe, tmp, name, img)
            assert out[name] is not None, name
        for (w, h, n), img in vc.chain_images().items():
            for step in range(1, n + 1):
                img = run_reference(exe, tmp, vc.chain_name(w, h, step), img)
                assert img is not None, (w, h, step)
                out[vc.chain_name(w, h, step)] = img
        w, h, c = vc.REFUSED_SHAPE
        out["refused"] = np.array(run_reference(exe, tmp, "refused", np.zeros((h, w), np.uint8)) is None)
    # an .npz whose bytes depend on its arrays alone: fixed entry order and time stamps
    with zipfile.ZipFile(vc.GOLDEN, "w") as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(vc.GOLDEN, os.path.getsize(vc.GOLDEN), "bytes")
    vc.golden.cache_clear()
    for name, img in vc.halve_images().items():
        assert vc.halve(img).tobytes() == vc.golden()[name].tobytes() and vc.halve(img).shape == vc.golden()[name].shape, name
    for (w, h, n), img in vc.chain_images().items():
        for step in range(1, n + 1):
            img = vc.halve(img)
            assert img.tobytes() == vc.golden()[vc.chain_name(w, h, step)].tobytes(), (w, h, step)
    print(len(out) - 1, "images: the restatement equals the reference")


if __name__ == "__main__":
    main()
