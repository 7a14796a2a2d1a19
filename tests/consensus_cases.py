"""Cases of the per-track consensus triangulation (osfm_ba_consensus; the definition is tests/consensus_restatement.py).

Both camera models, the smallest shapes that reach every path of orthosfm_amd/csrc/consensus_kernels.hip: tracks of at
most SHORT_LEN observations take eight lanes (SHORT_TRACKS tracks per workgroup), longer ones a wave (LONG_TRACKS per
workgroup); more than max_sample observations are sampled; 120 hypotheses take two rounds of 64 lanes; observations
are staged 64 at a time.
  planted      24 ring cameras x 300 tracks of 2..12 views, 0.3 px noise, ground-truth cameras; one random-pixel
               observation in 30 % of the tracks of 3 or more, two in 10 % of those of 6 or more, four in 4 % of those
               of 10 or more (exact shares of every length, so that each length has its contaminated tracks)
  lengths      the ring of tri_cases: lengths 2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 128, 129, 250, 260 with a
               track of 0 or 1 observations between each two; floor(0.3 n) wrong observations in every track of 4 or
               more, the first of them on observation 0 (always sampled) and on the last sampled index
  single_ok, single_bad
               M = 1, two rays that agree / that are 50 px apart
  degenerate_axis, degenerate_mix
               tri_cases' cameras with one exact axis direction (every pair parallel) / three of those and three
               ring cameras (tracks inside the first three are degenerate, the others not)
  intrinsics   tri_cases' case: images of 1920 x 1080 and 3 x 5, scales 0.37, 1 and 4, offsets +-0.3, its out-of-frame
               pixels as natural outliers
  max_error_0.75, max_error_3, min_support_2, min_support_4, refit_rounds_0, refit_rounds_1
               planted under other options
  max_sample_4 48 tracks of 5..9 views, one wrong observation in every third, max_sample = 4
  edges_short_31 .. 33, edges_long_3 .. 5
               M one below, at and one above the tracks of a workgroup: lengths 2..8 resp. 9..20
A Case holds the scene, the options, and where observations were planted: planted (O,) bool or None.
"""
import numpy as np

import tri_cases as tri
from orthosfm_amd import synth

Q, E = synth.MODEL_QUATERNION, synth.MODEL_EULER
SEED = synth.BASE_SEED
_ST = 0xC05 << 32
SHORT_LEN, SHORT_TRACKS, LONG_TRACKS, MAX_SAMPLE = 8, 32, 4, 16
LENGTHS = (2, 3, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 128, 129, 250, 260)


class Case:
    def __init__(self, sc, opts=None, planted=None):
        self.sc, self.opts, self.planted = sc, dict(opts or {}), planted


def _plant(sc, counts, stream, forced=None):
    """Replaces counts[j] observations of track j by pixels drawn over the whole image; forced[j]: positions that are
    taken first.  Returns the (O,) bool mask."""
    M, O = sc.points.shape[0], sc.obs_xy.shape[0]
    start = np.concatenate([[0], np.cumsum(tri.track_lengths(sc))]).astype(np.int64)
    order = synth.uniform(SEED, _ST | stream, O)
    pix = synth.uniform(SEED, _ST | (stream + 1), 2 * O).reshape(O, 2)
    planted = np.zeros(O, dtype=bool)
    for j in range(M):
        k0, k1, k = int(start[j]), int(start[j + 1]), int(counts[j])
        if k == 0:
            continue
        pos = [p for p in (forced[j] if forced else [])][:k]
        rest = [int(p) for p in np.argsort(order[k0:k1], kind="stable") if int(p) not in pos]
        pos = pos + rest[:k - len(pos)]
        planted[k0 + np.asarray(pos, dtype=np.int64)] = True
    c = sc.obs_camera[planted]
    sc.obs_xy[planted] = tri._f32(pix[planted] * np.stack([sc.img_w[c], sc.img_h[c]], axis=1))
    return planted


def _planted_counts(ln, stream):
    """Per length class, in the order of a drawn key: four wrong observations in 4 % of the tracks (lengths of 10 or
    more), two in the next 10 % (6 or more), one in the next 30 % (3 or more) -- exact shares, so that every class has
    its contaminated tracks whatever the draw."""
    ln = np.asarray(ln)
    u = synth.uniform(SEED, _ST | stream, len(ln))
    k = np.zeros(len(ln), dtype=np.int64)
    for n in np.unique(ln):
        cls = np.nonzero(ln == n)[0]
        cls = cls[np.argsort(u[cls], kind="stable")]
        n4 = int(round(0.04 * len(cls))) if n >= 10 else 0
        n2 = int(round(0.10 * len(cls))) if n >= 6 else 0
        n1 = int(round(0.30 * len(cls))) if n >= 3 else 0
        k[cls[:n4]], k[cls[n4:n4 + n2]], k[cls[n4 + n2:n4 + n2 + n1]] = 4, 2, 1
    return k


def _planted(model, opts=None):
    C, M = 24, 300
    cams = tri._ring(model, C, 0x110)
    ln = 2 + np.arange(M) % 11
    sc = tri._scene(model, cams, *tri._sizes(C), tri._ball(M, 0x112), tri._arcs(ln, C, 0x114), 0.3, 0x115)
    return Case(sc, opts, _plant(sc, _planted_counts(ln, 0x02), 0x03))


def _lengths(model):
    C = 260
    cams = tri._ring(model, C, 0x10)
    ln = []
    for i, n in enumerate(LENGTHS):
        ln.append(n)
        if i + 1 < len(LENGTHS):
            ln.append(i % 2)
    sc = tri._scene(model, cams, *tri._sizes(C), tri._ball(len(ln), 0x12), tri._arcs(ln, C, 0x14), 0.3, 0x15)
    counts = [int(0.3 * n) if n >= 4 else 0 for n in ln]
    forced = [[0, int(((MAX_SAMPLE - 1) * n) // MAX_SAMPLE) if n > MAX_SAMPLE else n - 1] for n in ln]
    return Case(sc, None, _plant(sc, counts, 0x10, forced))


def _single(model, shift):
    sc = tri.build("single", model)
    sc.obs_xy[1, 0] += shift
    return Case(sc)


def _degenerate_mix(model):
    C, M = 6, 48
    axis = tri.build("parallel_axis", model).cam_params[:3]
    ang = [(2.0 * np.pi * c / 5, 0.3 - 0.2 * c, 0.1 * c) for c in range(3)]
    cams = np.concatenate([axis, tri._cams_from_euler(model, ang, np.zeros((3, 2)), np.ones(3))])
    ln = [2 + j % 4 for j in range(M)]
    return Case(tri._scene(model, cams, *tri._sizes(C), tri._ball(M, 0x212), tri._arcs(ln, C, 0x214), 0.3, 0x215))


def _max_sample_4(model):
    C, M = 24, 48
    cams = tri._ring(model, C, 0x110)
    ln = np.array([5 + j % 5 for j in range(M)])
    sc = tri._scene(model, cams, *tri._sizes(C), tri._ball(M, 0x312), tri._arcs(ln, C, 0x314), 0.3, 0x315)
    return Case(sc, {"max_sample": 4}, _plant(sc, [1 if j % 3 == 0 else 0 for j in range(M)], 0x30))


def _edges(model, M, lo, hi, stream):
    C = 24
    cams = tri._ring(model, C, 0x110)
    ln = np.array([lo + j % (hi - lo + 1) for j in range(M)])
    sc = tri._scene(model, cams, *tri._sizes(C), tri._ball(M, stream), tri._arcs(ln, C, stream + 2), 0.3, stream + 3)
    return Case(sc, None, _plant(sc, [1 if n >= 4 and j % 2 else 0 for j, n in enumerate(ln)], stream + 4))


_BUILDERS = {
    "planted": _planted,
    "lengths": _lengths,
    "single_ok": lambda m: _single(m, 0.0),
    "single_bad": lambda m: _single(m, 50.0),
    "degenerate_axis": lambda m: Case(tri.build("parallel_axis", m)),
    "degenerate_mix": _degenerate_mix,
    "intrinsics": lambda m: Case(tri.build("intrinsics", m)),
    "max_error_0.75": lambda m: _planted(m, {"max_error": 0.75}),
    "max_error_3": lambda m: _planted(m, {"max_error": 3.0}),
    "min_support_2": lambda m: _planted(m, {"min_support": 2}),
    "min_support_4": lambda m: _planted(m, {"min_support": 4}),
    "refit_rounds_0": lambda m: _planted(m, {"refit_rounds": 0}),
    "refit_rounds_1": lambda m: _planted(m, {"refit_rounds": 1}),
    "max_sample_4": _max_sample_4,
}
for _M in (SHORT_TRACKS - 1, SHORT_TRACKS, SHORT_TRACKS + 1):
    _BUILDERS[f"edges_short_{_M}"] = lambda m, _M=_M: _edges(m, _M, 2, SHORT_LEN, 0x400 + 16 * _M)
for _M in (LONG_TRACKS - 1, LONG_TRACKS, LONG_TRACKS + 1):
    _BUILDERS[f"edges_long_{_M}"] = lambda m, _M=_M: _edges(m, _M, SHORT_LEN + 1, 20, 0x800 + 16 * _M)

NAMES = tuple(_BUILDERS)
ALL = [(name, model) for name in NAMES for model in (Q, E)]
_cache = {}


def build(name, model):
    """The Case, built once per process; its arrays are read-only."""
    key = (name, model)
    if key not in _cache:
        case = _BUILDERS[name](model)
        sc = case.sc
        assert (np.diff(sc.obs_point) >= 0).all()
        for a in (sc.cam_params, sc.points, sc.obs_xy, sc.obs_camera, sc.obs_point, sc.img_w, sc.img_h):
            a.setflags(write=False)
        _cache[key] = case
    return _cache[key]


_ref = {}


def restated(name, model):
    """consensus_restatement.consensus of the case under its options, computed once per process."""
    import consensus_restatement as cr
    key = (name, model)
    if key not in _ref:
        case = build(name, model)
        _ref[key] = cr.consensus(case.sc, **case.opts)
    return _ref[key]


def expected_keep(case, min_support=3):
    """The planted mask as keep flags, all zero on tracks where fewer than min_support (and, with two observations,
    fewer than two) good observations remain; tracks of fewer than two observations keep theirs."""
    sc = case.sc
    keep = ~case.planted
    start = np.concatenate([[0], np.cumsum(tri.track_lengths(sc))]).astype(np.int64)
    for j in range(sc.points.shape[0]):
        k0, k1 = int(start[j]), int(start[j + 1])
        n, good = k1 - k0, int(keep[k0:k1].sum())
        if n >= 2 and good < n and good < min_support:
            keep[k0:k1] = False
    return keep


def key(name, model):
    return f"{name}-{'quat' if model == Q else 'euler'}"
