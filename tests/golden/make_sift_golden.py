"""Writes tests/golden/sift_reference.npz: per case of tests/sift_cases.py what the reference SIFT detector makes of
the case's image, stage by stage -- the SHA-256 of the input, of every octave image and of every DoG image, the
candidate list, the localised keypoints, the descriptors with x, y, scale and orientation in generation order, and
the FeatureSet view (the permutation that sorts by scale, colours, normalised positions).  For the cases of
sift_cases.EDGE it keeps the hashes, the candidates, the keypoints and whether the reference threw, and checks that
every octave of at least sift_cases.MIN_SIDE pixels a side holds a candidate.

The reference is compiled here from its own sources (REF, default /root/reference) with the driver beside this file
into a temporary directory; nothing of it enters the tree.  The script then holds the numpy restatement
(tests/sift_restatement.py) against what it wrote, checks what each case must show, refuses a case with too many
ambiguous keypoints and prints the figures that tests/sift_cases.py records in MEASURED.

    python tests/golden/make_sift_golden.py [--time]      (--time: Sift::process on the 2048 x 2048 timing canvas)
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

import sift_cases as sc  # noqa: E402
import sift_restatement as sr  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
MVE = os.path.join(REF, "src", "mve")


def compile_driver(tmp):
    exe = os.path.join(tmp, "sift_golden_driver")
    subprocess.check_call(["g++", "-O2", "-msse3", "-std=c++11", "-fno-access-control", "-w",
                           "-DMVE_NO_PNG_SUPPORT", "-DMVE_NO_JPEG_SUPPORT", "-DMVE_NO_TIFF_SUPPORT", "-I" + MVE,
                           "-o", exe, os.path.join(HERE, "sift_golden_driver.cc"),
                           os.path.join(MVE, "sfm", "sift.cc"), os.path.join(MVE, "mve", "image_tools.cc")])
    return exe


def read_records(path):
    out = {}
    with open(path, "rb") as f:
        blob = f.read()
    p = 0
    while p < len(blob):
        n = int(np.frombuffer(blob, "<u4", 1, p)[0]); p += 4
        name = blob[p:p + n].decode(); p += n
        t = chr(blob[p]); p += 1
        rows, cols = (int(v) for v in np.frombuffer(blob, "<u4", 2, p)); p += 8
        dt = {"f": "<f4", "i": "<i4", "b": "u1"}[t]
        out[name] = np.frombuffer(blob, dt, rows * cols, p).reshape(rows, cols).copy()
        p += rows * cols * np.dtype(dt).itemsize
    return out


def run_reference(exe, tmp, case):
    img = sc.image(case.name)
    raw = os.path.join(tmp, case.name + ".raw")
    img.tofile(raw)
    out = os.path.join(tmp, case.name + ".bin")
    args = [exe, raw, str(case.width), str(case.height), str(case.channels), str(case.min_octave), out]
    if (case.samples, case.base_blur_sigma) != (3, 1.6):
        args += [str(case.samples), repr(case.base_blur_sigma)]
    subprocess.check_call(args)
    return read_records(out)


def fixture_of(case, rec):
    """The arrays the fixture keeps for one case."""
    fx = {"image_sha": np.array(sc.sha(sc.image(case.name))), "threw": rec["threw"].reshape(()).astype(np.int32)}
    if fx["threw"]:
        return fx
    n_oct = len({k.split("/")[1] for k in rec if k.startswith("img/")})
    S = case.samples
    fx["img_sha"] = np.array([[sc.sha(rec[f"img/{o}/{i}"]) for i in range(S + 3)] for o in range(n_oct)], dtype="S64")
    fx["dog_sha"] = np.array([[sc.sha(rec[f"dog/{o}/{i}"]) for i in range(S + 2)] for o in range(n_oct)], dtype="S64")
    fx["octave_shape"] = np.array([rec[f"img/{o}/0"].shape for o in range(n_oct)], dtype=np.int32)
    fx["candidates"] = rec["candidates"].astype(np.float32).reshape(-1, 4)
    fx["keypoints"] = rec["keypoints"].astype(np.float32).reshape(-1, 4)
    if case.name in sc.EDGE:            # stage hashes, candidates, keypoints and the refused flag alone
        return fx
    fx["gen_meta"] = rec["gen/meta"].reshape(-1, 4)
    fx["gen_data"] = rec["gen/data"].reshape(-1, 128)
    # the sorted view as a permutation of the generation order (rows are told apart by their bytes)
    key = lambda m, d, i: m[i].tobytes() + d[i].tobytes()
    where = {}
    for i in range(len(fx["gen_meta"])):
        where.setdefault(key(fx["gen_meta"], fx["gen_data"], i), []).append(i)
    sm, sd = rec["sorted/meta"].reshape(-1, 4), rec["sorted/data"].reshape(-1, 128)
    fx["sorted_perm"] = np.array([where[key(sm, sd, i)].pop(0) for i in range(len(sm))], dtype=np.int32)
    fx["sorted_colors"] = rec["sorted/colors"].reshape(-1, 3)
    fx["sorted_normalized"] = rec["sorted/normalized"].reshape(-1, 2)
    return fx


def check_case(case, fx):
    """Holds the restatement against the fixture and returns the measured figures of the case."""
    opts = sc.options(case)
    assert bool(fx["threw"]) == case.refused == sr.refuses(case.width, case.height, opts), case.name
    if case.refused:
        print(f"{case.name:8s} the reference throws")
        return None
    octs = sr.scale_space(sc.image(case.name), opts)
    assert [[sc.sha(i) for i in o[1]] for o in octs] == fx["img_sha"].astype(str).tolist(), f"{case.name}: octave images differ"
    assert [[sc.sha(i) for i in o[2]] for o in octs] == fx["dog_sha"].astype(str).tolist(), f"{case.name}: DoG images differ"
    cand = sr.extrema(octs)
    assert cand.tobytes() == fx["candidates"].tobytes(), f"{case.name}: candidates differ"
    kps, rejected, moved, singular = sr.localise(octs, cand, opts)
    assert kps.tobytes() == fx["keypoints"].tobytes(), f"{case.name}: keypoints differ"
    per_oct = {int(o): int((kps[:, 0] == o).sum()) for o in np.unique(kps[:, 0])}
    fired = rejected.sum(0)
    n_desc = len(fx["gen_meta"]) if "gen_meta" in fx else "not kept"
    print(f"{case.name:8s} candidates {len(cand)} keypoints {len(kps)} per octave {per_oct} descriptors {n_desc} "
          f"moved {int(moved.sum())} singular {int(singular.sum())}")
    print(f"{'':8s} rejections " + ", ".join(f"{n} {int(c)}" for n, c in zip(sr.REJECTION_TESTS, fired))
          + "; never fired: " + (", ".join(n for n, c in zip(sr.REJECTION_TESTS, fired) if not c) or "none"))
    if case.name in sc.EDGE:
        sides = {o[0]: min(o[1][0].shape) for o in octs}
        assert all((cand[:, 0] == o).any() for o, side in sides.items() if side >= sc.MIN_SIDE), f"{case.name}: an octave without candidates"
        return None
    if not case.descriptors:
        assert len(fx["gen_meta"]) == 0, f"{case.name} has descriptors: hold it to the descriptor checks"
        return None
    fig = sc.measure(case.name)
    print(f"{'':8s} d_ori {fig['d_ori']:.3e} d_desc {fig['d_desc']:.3e} ambiguous {fig['ambiguous']} of {len(kps)} "
          f"({100.0 * fig['ambiguous'] / max(1, len(kps)):.2f} %), several orientations {fig['several']}, "
          f"float32 restatement: count differs on {fig['f32_count_differs']} clear keypoints")
    assert fig["ambiguous"] <= 0.02 * len(kps), f"{case.name}: too many ambiguous keypoints, pick another seed"
    assert fig["f32_count_differs"] == 0, f"{case.name}: the float32 restatement disagrees on a clear keypoint"
    if case.name == "base":
        assert all(per_oct.get(o, 0) >= 1 for o in (0, 1, 2)), per_oct
        assert moved.any() and fig["several"] >= 3
    if case.name == "many":
        assert len(cand) > 512
    return fig


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        if "--time" in sys.argv:
            raw = os.path.join(tmp, "canvas.raw")
            sc.timing_canvas().tofile(raw)
            print(subprocess.check_output([exe, raw, "2048", "2048", "1", "0", "--time", "3"], text=True).strip())
            return
        out, figures = {}, {}
        for case in sc.CASES:
            fx = fixture_of(case, run_reference(exe, tmp, case))
            for k, v in fx.items():
                out[f"{case.name}/{k}"] = v
    # an .npz whose bytes depend on its arrays alone: fixed entry order and time stamps
    with zipfile.ZipFile(sc.GOLDEN, "w") as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(sc.GOLDEN, os.path.getsize(sc.GOLDEN), "bytes")
    sc.golden.cache_clear()
    for case in sc.CASES:
        fx = {k.split("/", 1)[1]: v for k, v in sc.golden().items() if k.startswith(case.name + "/")}
        fig = check_case(case, fx)
        if fig and case.descriptors:
            figures[case.name] = fig
    print("MEASURED = {")
    for n, f in figures.items():
        print(f"    \"{n}\": ({f['d_ori']:.3e}, {f['d_desc']:.3e}, {f['ambiguous']}, {f['keypoints']}),")
    print("}")


if __name__ == "__main__":
    main()
