"""tests/golden/cfg1_suzanne.npz (BASELINE configs[0]) is what its generator makes from the reference's
resources/Suzanne.ply (kept beside it as tests/golden/suzanne.ply.gz) and the test bench's camera draw --
checked again here by running the generator, and the fixture is checked for its shape."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "cfg1_suzanne.npz")


def test_fixture_shape():
    g = np.load(FIX)
    pts, cams = g["points"], g["cams_deg"]
    assert pts.shape == (7872, 3) and pts.dtype == np.float64
    assert cams.shape == (16, 3) and np.all(cams[0] == 0)
    assert np.array_equal(cams[:, 0], 22.5 * np.arange(16))             # dataset_generation.cpp:21-31
    assert np.all(np.abs(cams[1:, 1:]) <= 30.0)
    assert np.abs(pts).max() < 0.5                                       # the model fits the unit cube the cameras look at


def test_fixture_equals_generator_output(tmp_path):
    # the generator writes next to itself: run a copy (with the mesh it reads) in a scratch folder
    gen = os.path.join(HERE, "golden", "make_cfg1_suzanne.py")
    work = tmp_path / "golden"
    work.mkdir()
    (work / "make_cfg1_suzanne.py").write_text(open(gen).read())
    (work / "suzanne.ply.gz").write_bytes(open(os.path.join(HERE, "golden", "suzanne.ply.gz"), "rb").read())
    subprocess.check_call([sys.executable, str(work / "make_cfg1_suzanne.py")], stdout=subprocess.DEVNULL)
    a, b = np.load(FIX), np.load(work / "cfg1_suzanne.npz")
    for k in ("points", "cams_deg", "width", "height"):
        assert np.array_equal(a[k], b[k]), k


def test_suzanne_scene_projects_into_the_image():
    sys.path.insert(0, os.path.join(HERE, ".."))
    from orthosfm_amd import synth
    sc = synth.make_suzanne_ba_scene(0, 3)
    assert sc.obs_xy.shape == (3 * 7872, 2)
    assert sc.obs_xy.min() > 0 and sc.obs_xy.max() < 2048
    # Euler and quaternion parametrisations of the same cameras see the same pixels
    se = synth.make_suzanne_ba_scene(1, 3)
    assert np.abs(sc.obs_xy - se.obs_xy).max() < 1e-3
