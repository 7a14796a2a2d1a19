"""Writes tests/golden/surf_reference.npz: per case of tests/surf_cases.py what the reference SURF detector makes of
the case's image, stage by stage -- the SHA-256 of the desaturated image and of the 16 response maps, the candidate
list, the localised keypoints, the descriptors with x, y, scale and orientation in generation order, the sine and
cosine the driver's C library gives for each orientation, and the FeatureSet view (the permutation that sorts by
scale, colours, normalised positions).  For `big` also descriptor_computation called directly on the hand-placed
inputs of surf_cases.forced().

The reference is compiled here from its own sources (REF, default /root/reference) with the driver beside this file
into a temporary directory; nothing of it enters the tree.  The script then holds the numpy restatement
(tests/surf_restatement.py) against what it wrote, refuses a case with more than 2 % ambiguous keypoints and prints
the figures that tests/surf_cases.py records in MEASURED.

    python tests/golden/make_surf_golden.py [--time]   (--time: set_image + Surf::process on the 2048 x 2048 timing canvas)
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
import surf_cases as uc  # noqa: E402
import surf_restatement as sr  # noqa: E402
from make_sift_golden import read_records  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
MVE = os.path.join(REF, "src", "mve")


def compile_driver(tmp):
    exe = os.path.join(tmp, "surf_golden_driver")
    subprocess.check_call(["g++", "-O2", "-msse3", "-std=c++11", "-fno-access-control", "-w",
                           "-DMVE_NO_PNG_SUPPORT", "-DMVE_NO_JPEG_SUPPORT", "-DMVE_NO_TIFF_SUPPORT", "-I" + MVE,
                           "-o", exe, os.path.join(HERE, "surf_golden_driver.cc"),
                           os.path.join(MVE, "sfm", "surf.cc"), os.path.join(MVE, "mve", "image_tools.cc")])
    return exe


def run_reference(exe, tmp, case):
    raw = os.path.join(tmp, case.name + ".raw")
    uc.image(case.name).tofile(raw)
    forced = "-"
    if case.name == "big":
        forced = os.path.join(tmp, "forced.f32")
        check_forced_taps()
        uc.forced().tofile(forced)
    out = os.path.join(tmp, case.name + ".bin")
    subprocess.check_call([exe, raw, str(case.width), str(case.height), str(case.channels), repr(case.contrast_threshold),
                           str(int(case.upright)), forced, out])
    return read_records(out)


def check_forced_taps():
    """No hand-placed descriptor may make the reference read beyond its table (undefined there)."""
    sat = sr.integral(sr.grey_of(uc.image("big")))
    for x, y, scale, ori, upright in uc.forced():
        s, c = (0.0, 1.0) if upright else (sr.sinf(ori), sr.cosf(ori))
        assert sr.describe(sat, x, y, scale, s, c)[0] != 2


def fixture_of(case, rec):
    fx = {"image_sha": np.array(sc.sha(uc.image(case.name))), "grey_sha": np.array(sc.sha(rec["grey"]))}
    fx["map_sha"] = np.array([[sc.sha(rec[f"map/{o}/{k}"]) for k in range(4)] for o in range(4)], dtype="S64")
    fx["map_shape"] = np.array([rec[f"map/{o}/0"].shape for o in range(4)], dtype=np.int32)
    fx["candidates"] = rec["candidates"].astype(np.float32).reshape(-1, 4)
    fx["keypoints"] = rec["keypoints"].astype(np.float32).reshape(-1, 4)
    fx["gen_meta"] = rec["gen/meta"].reshape(-1, 4)
    fx["gen_data"] = rec["gen/data"].reshape(-1, 64)
    fx["gen_trig"] = rec["gen/trig"].reshape(-1, 2)
    key = lambda m, d, i: m[i].tobytes() + d[i].tobytes()
    where = {}
    for i in range(len(fx["gen_meta"])):
        where.setdefault(key(fx["gen_meta"], fx["gen_data"], i), []).append(i)
    sm, sd = rec["sorted/meta"].reshape(-1, 4), rec["sorted/data"].reshape(-1, 64)
    fx["sorted_perm"] = np.array([where[key(sm, sd, i)].pop(0) for i in range(len(sm))], dtype=np.int32)
    fx["sorted_colors"] = rec["sorted/colors"].reshape(-1, 3)
    fx["sorted_normalized"] = rec["sorted/normalized"].reshape(-1, 2)
    if case.name == "big":
        assert rec["forced/in"].tobytes() == uc.forced().tobytes()
        fx["forced_ok"] = rec["forced/ok"].reshape(-1)
        fx["forced_data"] = rec["forced/data"].reshape(-1, 64)
        fx["forced_trig"] = rec["forced/trig"].reshape(-1, 2)
        fx["forced_coords"] = rec["forced/coords"].reshape(-1, 400, 2).astype(np.int16)
    return fx


def check_case(case):
    """Holds the restatement against the fixture and returns the measured figures of the case."""
    fx = uc.fixture(case.name)
    sat, maps, cand, kps, gen = uc.restated(case.name, True)
    assert sc.sha(sr.grey_of(uc.image(case.name))) == str(fx["grey_sha"])
    assert [[sc.sha(m) for m in o] for o in maps] == fx["map_sha"].astype(str).tolist(), f"{case.name}: maps differ"
    assert cand.tobytes() == fx["candidates"].tobytes(), f"{case.name}: candidates differ"
    assert kps.tobytes() == fx["keypoints"].tobytes(), f"{case.name}: keypoints differ"
    rows = uc.generation_rows(gen)
    per_oct = [int((kps[:, 0] == o).sum()) for o in range(4)]
    n_amb, n_ori = uc.measure(case.name)
    share = 100.0 * n_amb / max(1, n_ori)
    print(f"{case.name:8s} candidates {len(cand)} keypoints {len(kps)} per octave {per_oct} descriptors {len(fx['gen_meta'])} "
          f"scales {sorted({float(m[2]) for m in fx['gen_meta']})}")
    print(f"{'':8s} ambiguous {n_amb} of {n_ori} keypoints with an orientation ({share:.2f} %), guarded "
          f"{sum(r['status'] == 2 for r in rows)}")
    assert n_amb <= 0.02 * max(1, n_ori), f"{case.name}: too many ambiguous keypoints, pick another seed"
    if case.name in uc.EDGE:
        assert all((cand[:, 0] == o).any() for o in uc.capable_octaves(case.width, case.height)), f"{case.name}: an octave without candidates"
    if case.counts:
        got = (len(cand), len(kps), len(fx["gen_meta"]))
        assert all(w is None or w == g for w, g in zip(case.counts, got)), (case.name, got)
    clear = [r for r in rows if not r["ambiguous"]]
    if all(not g["ambiguous"] for g in gen if g is not None):
        assert len(rows) == len(fx["gen_meta"])
        meta = np.array([[r["x"], r["y"], r["scale"], r["orientation"]] for r in rows], np.float32).reshape(-1, 4)
        assert meta.tobytes() == fx["gen_meta"].tobytes(), f"{case.name}: x, y, scale or orientation differ"
        assert np.array([r["data"] for r in rows], np.float32).reshape(-1, 64).tobytes() == fx["gen_data"].tobytes(), case.name
    else:
        print(f"{'':8s} {len(clear)} of {len(rows)} descriptors belong to clear keypoints")
    return n_amb, n_ori


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_driver(tmp)
        if "--time" in sys.argv:
            raw = os.path.join(tmp, "canvas.raw")
            sc.timing_canvas().tofile(raw)
            print(subprocess.check_output([exe, raw, "2048", "2048", "1", "500", "0", "--time", "3"], text=True).strip())
            return
        out = {}
        for case in uc.CASES:
            for k, v in fixture_of(case, run_reference(exe, tmp, case)).items():
                out[f"{case.name}/{k}"] = v
    # an .npz whose bytes depend on its arrays alone: fixed entry order and time stamps
    with zipfile.ZipFile(uc.GOLDEN, "w") as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(uc.GOLDEN, os.path.getsize(uc.GOLDEN), "bytes")
    uc.golden.cache_clear()
    figures = {case.name: check_case(case) for case in uc.CASES}
    print("MEASURED = {")
    for n, (a, k) in figures.items():
        print(f"    \"{n}\": ({a}, {k}),")
    print("}")


if __name__ == "__main__":
    main()
