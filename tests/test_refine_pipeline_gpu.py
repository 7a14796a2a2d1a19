"""tracks_from_images(refine=True) against refine=False on three rendered 512 x 512 views of one textured plane (a
plane suffices: only matching and tracks are exercised).  The views are affine images of the plane, so the exact
correspondence of every detector position is known."""
import numpy as np
import pytest

import refine_cases as rc
from orthosfm_amd import capi, pipeline

pytestmark = pytest.mark.gpu

SIZE = 512


def _views():
    c = (SIZE / 2.0, SIZE / 2.0)
    return [rc.make_view(SIZE, SIZE, np.eye(2), centre=c), rc.make_view(SIZE, SIZE, 0.95 * rc.rot(0.05), centre=c, gain=0.9),
            rc.make_view(SIZE, SIZE, rc.rot(-0.04) / 0.96, centre=c, gain=1.1, bias=0.02)]


def _render(view, blobs):
    """Gaussian blobs (centre, covariance, amplitude on the plane) under the view's map: the centre maps by M, the
    covariance by M C M^T; every blob is added on its own 4.5 sigma box.  uint8 [SIZE, SIZE]."""
    acc = np.zeros((view.height, view.width))
    for cx, cy, c00, c01, c11, amp in blobs:
        mu = view.M @ np.array([cx, cy]) + view.t
        S = view.M @ np.array([[c00, c01], [c01, c11]]) @ view.M.T
        reach = 4.5 * np.sqrt(max(S[0, 0], S[1, 1]))
        x0, x1 = max(int(mu[0] - reach), 0), min(int(mu[0] + reach) + 2, view.width)
        y0, y1 = max(int(mu[1] - reach), 0), min(int(mu[1] + reach) + 2, view.height)
        if x0 >= x1 or y0 >= y1:
            continue
        P = np.linalg.inv(S)
        dx, dy = np.arange(x0, x1)[None, :] - mu[0], np.arange(y0, y1)[:, None] - mu[1]
        acc[y0:y1, x0:x1] += amp * np.exp(-0.5 * (P[0, 0] * dx * dx + 2.0 * P[0, 1] * dx * dy + P[1, 1] * dy * dy))
    return np.clip(np.floor((0.5 + view.gain * acc + view.bias) * 255.0 + 0.5), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene():
    n = 5000
    u = rc._u(301, 11, 7 * n).reshape(n, 7)
    s1 = 1.6 * (4.0 / 1.6) ** u[:, 2]
    s2 = s1 * (0.6 + 0.4 * u[:, 3])
    ca, sa = np.cos(np.pi * u[:, 4]), np.sin(np.pi * u[:, 4])
    blobs = np.stack([-60.0 + u[:, 0] * (SIZE + 120.0), -60.0 + u[:, 1] * (SIZE + 120.0),
                      ca * ca * s1 * s1 + sa * sa * s2 * s2, ca * sa * (s1 * s1 - s2 * s2), sa * sa * s1 * s1 + ca * ca * s2 * s2,
                      (0.05 + 0.15 * u[:, 5]) * np.where(u[:, 6] < 0.5, -1.0, 1.0)], axis=1)
    views = _views()
    images = [_render(v, blobs) for v in views]
    plain = pipeline.tracks_from_images(images, verify=False)
    off = pipeline.tracks_from_images(images, verify=False, refine=False)
    tm = pipeline.Timings()
    on = pipeline.tracks_from_images(images, verify=False, refine=True, timings=tm)
    return views, plain, off, on, tm


def _table_bytes(tt):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (tt.offsets, tt.view, tt.feat, tt.xy))


def test_refine_false_changes_nothing(scene):
    _, plain, off, _, _ = scene
    assert _table_bytes(plain[0]) == _table_bytes(off[0])
    assert plain[1].tobytes() == off[1].tobytes()
    assert "refine" not in off[2]


def test_refined_rows_move_and_no_others(scene):
    _, _, off, on, tm = scene
    a, b, info = off[0], on[0], on[2]["refine"]
    assert a.offsets.tobytes() == b.offsets.tobytes() and a.view.tobytes() == b.view.tobytes() and a.feat.tobytes() == b.feat.tobytes()
    assert off[1].tobytes() == on[1].tobytes()
    status = info["status"]
    assert status.shape == (a.view.shape[0],)
    moved = (a.xy != b.xy).any(axis=1)
    assert np.array_equal(moved, status == capi.REFINE_REFINED)
    assert np.array_equal(b.xy, b.xy.astype(np.float32).astype(np.float64))         # float32 values, as Feature::x/y
    for i, key in enumerate(capi.REFINE_STATUS):
        assert info[key] == int((status == i).sum())
    assert info["reference"] == a.offsets.shape[0] - 1 and info["device_ms"] > 0.0 and tm.refine_s > 0.0


def test_true_matches_get_closer(scene):
    """Over the observations whose detector position lies within 3 px of the exact correspondence of their track's
    reference observation: the median distance to it falls, and at least half of them are REFINED."""
    views, _, off, on, _ = scene
    a, b, status = off[0], on[0], on[2]["refine"]["status"]
    assert a.offsets.shape[0] - 1 > 100
    ref = np.repeat(a.offsets[:-1], np.diff(a.offsets))
    other = np.flatnonzero(np.arange(a.view.shape[0]) != ref)
    # table pixels are image pixels + 0.5 here: import width = feature width = max side = SIZE
    M = np.stack([v.M for v in views])
    t = np.stack([v.t for v in views])
    X = np.linalg.solve(M[a.view[ref[other]]], (a.xy[ref[other]] - 0.5 - t[a.view[ref[other]]])[:, :, None])[:, :, 0]
    truth = np.einsum("nij,nj->ni", M[a.view[other]], X) + t[a.view[other]] + 0.5
    before = np.linalg.norm(a.xy[other] - truth, axis=1)
    after = np.linalg.norm(b.xy[other] - truth, axis=1)
    true = before < 3.0
    assert true.sum() > 100
    transfer_before, transfer_after = float(np.median(before[true])), float(np.median(after[true]))
    refined = float((status[other][true] == capi.REFINE_REFINED).mean())
    print(f"true matches {int(true.sum())} of {other.size}: transfer_before {transfer_before:.4f} px, transfer_after "
          f"{transfer_after:.4f} px, refined {refined:.3f}")
    assert transfer_after < transfer_before
    assert refined >= 0.5
