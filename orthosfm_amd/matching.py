"""Host-side mirror of the reference's matcher plug-in interface on top of
the C ABI: sfm::MatchingBase { init, pairwise_match, pairwise_match_lowres }
(src/mve/sfm/matching_base.h:22-55) and the all-pairs driver
sfm::bundler::Matching::compute (src/mve/sfm/bundler_matching.cc:58-136,
up to the RANSAC stage).  Same names, argument meaning and error behaviour
(exceptions for invalid arguments, -1 for unsuccessful matches).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import capi


@dataclass
class MatchResult:
    """sfm::Matching::Result (src/mve/sfm/matching.h:56-62)."""
    matches_1_2: np.ndarray
    matches_2_1: np.ndarray


_PAIR_RESULT_DTYPE = np.dtype([("status", np.int32), ("lowres_matches", np.int32), ("num_matches", np.int32),
                               ("num_inliers", np.int32), ("offset", np.int64)])
assert _PAIR_RESULT_DTYPE.itemsize == C.sizeof(capi.PairResult)
_GUIDED_RESULT_DTYPE = np.dtype([("status", np.int32), ("num_seeds", np.int32), ("num_added", np.int32),
                                 ("max_candidates", np.int32), ("offset", np.int64)])
assert _GUIDED_RESULT_DTYPE.itemsize == C.sizeof(capi.GuidedResult)


@dataclass
class TwoViewMatching:
    """sfm::bundler::TwoViewMatching (bundler_common.h:118-125) before RANSAC."""
    view_1_id: int
    view_2_id: int
    matches: np.ndarray          # (k, 2) int32 (feature in view 1, feature in view 2)
    status: int = 0
    lowres_matches: int = -1
    num_matches: int = 0
    num_inliers: int = -1


class HipExhaustiveMatching:
    """Drop-in for sfm::ExhaustiveMatching (src/mve/sfm/exhaustive_matching.h:26-66)
    backed by the gfx950 kernels."""

    def __init__(self, num_views: int, device=0, options: capi.MatchOptions | None = None,
                 copy_results: bool = True):
        """copy_results=False: the lists compute() returns are views into a buffer
        the matcher reuses -- valid until the next compute() (no second pass over
        the results on the host).  device: one device id, or a sequence of them
        (osfm_match_create_multi: the bank on every device, the pairs of compute() dealt
        over them by work; an id may repeat -- logical shards on one device)."""
        self.opts = options if options is not None else capi.default_match_options()
        self._copy_results = bool(copy_results)
        self._h = C.c_void_p()
        if isinstance(device, (list, tuple, np.ndarray)):
            ids = (C.c_int * len(device))(*[int(d) for d in device])
            capi.check(capi.lib.osfm_match_create_multi_v2(ids, len(device), num_views, C.byref(self.opts), C.byref(self._h)))
        else:
            capi.check(capi.lib.osfm_match_create_v2(int(device), num_views, C.byref(self.opts), C.byref(self._h)))
        self.num_views = num_views

    def devices(self):
        """The device of every shard (osfm_match_get_devices)."""
        ids = (C.c_int32 * 64)()
        n = C.c_int32()
        capi.check(capi.lib.osfm_match_get_devices(self._h, ids, 64, C.byref(n)))
        return [int(ids[k]) for k in range(min(n.value, 64))]

    # --- MatchingBase::init ---------------------------------------------------
    def init(self, viewports):
        """viewports: sequence of (sift_float[n,128], surf_float[m,64]) -- the
        FeatureSet::sift_descriptors / surf_descriptors data rows."""
        if viewports is None:
            raise ValueError("Viewports must not be null")   # bundler_matching.cc:47-48
        for v, (sift, surf) in enumerate(viewports):
            self.set_view_float(v, sift, surf)

    def set_view_float(self, view, sift, surf):
        sift = np.ascontiguousarray(sift, dtype=np.float32).reshape(-1, 128)
        surf = np.ascontiguousarray(surf, dtype=np.float32).reshape(-1, 64)
        capi.check(capi.lib.osfm_match_set_view_float(
            self._h, view, capi._ptr(sift, C.c_float), sift.shape[0],
            capi._ptr(surf, C.c_float), surf.shape[0]))

    def set_view(self, view, sift_u16, surf_s16=None):
        sift = np.ascontiguousarray(sift_u16, dtype=np.uint16).reshape(-1, 128)
        surf = (np.zeros((0, 64), np.int16) if surf_s16 is None
                else np.ascontiguousarray(surf_s16, dtype=np.int16).reshape(-1, 64))
        capi.check(capi.lib.osfm_match_set_view(
            self._h, view, capi._ptr(sift, C.c_uint16), sift.shape[0],
            capi._ptr(surf, C.c_int16), surf.shape[0]))

    def set_view_features(self, view, features):
        """A view from features.SiftExtractor.extract (its descriptors and its normalised positions) or from
        features.FeatureSetExtractor.extract (SIFT and SURF descriptors, and the positions of both, SIFT first)."""
        if hasattr(features, "sift") and hasattr(features, "surf"):
            self.set_view_float(view, features.sift.descriptors, features.surf.descriptors)
        else:
            self.set_view_float(view, features.descriptors, np.zeros((0, 64), np.float32))
        self.set_positions(view, features.normalized)

    def set_view_from_front(self, view, front):
        """A view from the last load of a features.ViewFrontEnd, on the device (osfm_match_set_view_from_front): the
        bank and the positions that set_view_features(view, front.download()) would leave, without the descriptors'
        way through the host."""
        capi.check(capi.lib.osfm_match_set_view_from_front(self._h, int(view), front._h))

    # --- test hooks ---------------------------------------------------------------------------------------------
    _BANK_DTYPES = {"sift": np.int8, "sift_raw": np.int8, "special": np.int8, "surf": np.int8, "positions": np.float32}

    def debug_view_bank(self, view, shard=0):
        """osfm_match_debug_view_bank: a dictionary of the view's counts and of every array a matching call reads."""
        b = capi.ViewBank()
        capi.check(capi.lib.osfm_match_debug_view_bank(self._h, int(view), int(shard), C.byref(b)))
        sp = b.n_special > 0
        length = {"sift": b.n_sift_pad * 128, "sift_raw": b.n_sift_pad * 128, "sift_corr": b.n_sift_pad, "sift_raw_corr": b.n_sift_pad,
                  "surf": b.n_surf_pad * 64, "surf_corr": b.n_surf_pad, "special": b.n_special_pad * 128,
                  "special_corr": b.n_special_pad, "special_map": b.n_special if sp else 0, "special_slot": b.n_sift if sp else 0,
                  "positions": max(b.n_positions, 0) * 2}
        out = {n: np.zeros(length[n], self._BANK_DTYPES.get(n, np.int32)) for n in capi.ViewBank.ARRAYS}
        for n, a in out.items():
            setattr(b, n, a.ctypes.data if a.size else None)
        capi.check(capi.lib.osfm_match_debug_view_bank(self._h, int(view), int(shard), C.byref(b)))
        out.update({n: int(getattr(b, n)) for n in capi.ViewBank.COUNTS})
        return out

    def debug_set_view_device(self, view, sift, sift_order, surf, surf_order, positions):
        """osfm_match_debug_set_view_device: float rows (and optional permutations) through the device hand-off."""
        sift = np.ascontiguousarray(sift, dtype=np.float32).reshape(-1, 128)
        surf = np.ascontiguousarray(surf, dtype=np.float32).reshape(-1, 64)
        so = None if sift_order is None else np.ascontiguousarray(sift_order, dtype=np.int32)
        uo = None if surf_order is None else np.ascontiguousarray(surf_order, dtype=np.int32)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 2)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        capi.check(capi.lib.osfm_match_debug_set_view_device(self._h, int(view), ptr(sift), sift.shape[0], ptr(so), ptr(surf),
                                                             surf.shape[0], ptr(uo), ptr(pos)))

    def expect_pairs(self, pairs_per_call: int):
        """The largest compute() call to come: the work arrays are sized for it at once (osfm_match_expect_pairs)."""
        capi.check(capi.lib.osfm_match_expect_pairs(self._h, C.c_int32(int(pairs_per_call))))

    def set_positions(self, view, xy):
        """FeatureSet::positions (normalised x, y per feature) for RANSAC-F."""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        capi.check(capi.lib.osfm_match_set_positions(self._h, view, capi._ptr(xy, C.c_float), xy.shape[0]))

    def view_size(self, view):
        a, b = C.c_int(), C.c_int()
        capi.check(capi.lib.osfm_match_view_size(self._h, view, C.byref(a), C.byref(b)))
        return a.value, b.value

    # --- MatchingBase::pairwise_match -----------------------------------------
    def pairwise_match(self, view_1_id, view_2_id) -> MatchResult:
        n1 = sum(self.view_size(view_1_id))
        n2 = sum(self.view_size(view_2_id))
        m12 = np.full(max(n1, 1), -7, dtype=np.int32)
        m21 = np.full(max(n2, 1), -7, dtype=np.int32)
        l12, l21 = C.c_int32(), C.c_int32()
        capi.check(capi.lib.osfm_match_pair(
            self._h, view_1_id, view_2_id, capi._ptr(m12, C.c_int32), C.byref(l12),
            capi._ptr(m21, C.c_int32), C.byref(l21)))
        return MatchResult(m12[:l12.value].copy(), m21[:l21.value].copy())

    # --- MatchingBase::pairwise_match_lowres ----------------------------------
    def pairwise_match_lowres(self, view_1_id, view_2_id, num_features) -> int:
        c = C.c_int32()
        capi.check(capi.lib.osfm_match_pair_lowres(self._h, view_1_id, view_2_id, num_features, C.byref(c)))
        return c.value

    # --- Matching::twoway_match (matching.h:148-159), one descriptor type -------
    def twoway_match(self, view_1_id, view_2_id, descriptor_type=0, num_features=0) -> MatchResult:
        n1 = self.view_size(view_1_id)[descriptor_type]
        n2 = self.view_size(view_2_id)[descriptor_type]
        if num_features > 0:
            n1, n2 = min(n1, num_features), min(n2, num_features)
        m12 = np.full(max(n1, 1), -7, dtype=np.int32)
        m21 = np.full(max(n2, 1), -7, dtype=np.int32)
        capi.check(capi.lib.osfm_match_twoway(self._h, view_1_id, view_2_id, descriptor_type,
                                              num_features, capi._ptr(m12, C.c_int32),
                                              capi._ptr(m21, C.c_int32)))
        return MatchResult(m12[:n1].copy(), m21[:n2].copy())

    # --- bundler::Matching::compute (pre-RANSAC part), batched ----------------
    def compute_arrays(self, pairs=None, capacity=None):
        """osfm_match_all as it is: returns (records, corr) -- one record per input pair (status,
        lowres_matches, num_matches, num_inliers, offset: numpy fields of osfm_pair_result) and the
        (rows, 2) buffer all lists lie in, pair k at corr[offset : offset + count].  `pairs` may be
        an (n, 2) int32 array; the marshalled form of the last pair list is kept and reused when
        the CONTENT is the same (a list mutated in place is marshalled again).  The records are a
        fresh array per call; as_objects() takes the pair list from the call it is given."""
        if pairs is None:
            pairs = [capi.pair_from_index(i) for i in range(self.num_views * (self.num_views - 1) // 2)]
        flat = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        cached = getattr(self, "_pairs_cache", None)
        if cached is not None and cached[1].shape == flat.shape and np.array_equal(cached[1], flat):
            arr, flat = cached
        else:
            n = flat.shape[0]
            arr = (capi.Pair * max(n, 1))()
            flat = flat.copy()
            if n:
                np.ctypeslib.as_array(C.cast(arr, C.POINTER(C.c_int32)), shape=(n, 2))[:] = flat
            self._pairs_cache = (arr, flat)
        n = flat.shape[0]
        res = (capi.PairResult * max(n, 1))()
        if capacity is None:
            capacity = sum(min(sum(self.view_size(a)), sum(self.view_size(b))) for a, b in flat.tolist())
        # One result buffer per call, taken from a pool the matcher keeps (its pages
        # stay mapped, so the device-to-host copy does not fault them in again);
        # the per-pair lists are views into it.
        corr = self._take_buffer(max(capacity, 1))
        total = C.c_int64()
        capi.check(capi.lib.osfm_match_all(self._h, arr, n, res, capi._ptr(corr, C.c_int32),
                                           C.c_int64(capacity), C.byref(total)))
        corr = corr[:max(int(total.value), 0)].copy() if self._copy_results else corr
        # all lists of the call, concatenated in pair order (what the per-pair views point into)
        self.last_flat = corr[:max(int(total.value), 0)]
        ra = np.frombuffer(res, dtype=_PAIR_RESULT_DTYPE, count=n)      # keeps `res` alive; one per call
        self._last_pairs_flat = flat
        return ra, corr

    # --- guided matching inside the affine epipolar band (no counterpart in the reference) ---
    def guided_match(self, pairs, seed_offsets, seed_corr, F=None, capacity=None, **options):
        """osfm_match_guided as it is.  pairs (n, 2); seed_offsets (n + 1,) in correspondences; seed_corr (rows, 2);
        F None (fitted to each pair's seeds) or (n, 3, 3) in ransac_affine's layout; options: the fields of
        osfm_guided_options.  Returns (records, corr, F_used): one osfm_guided_result per pair as a numpy record, the
        (total, 2) lists (pair k at corr[offset : offset + num_seeds + num_added]) and the (n, 3, 3) F of every pair."""
        flat = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        n = flat.shape[0]
        off = np.ascontiguousarray(seed_offsets, dtype=np.int64).reshape(-1)
        assert off.shape[0] == n + 1, "guided_match: seed_offsets holds one entry more than there are pairs"
        seeds = np.ascontiguousarray(seed_corr, dtype=np.int32).reshape(-1, 2)
        o = capi.default_guided_options()
        for k, v in options.items():
            if k not in ("threshold", "sift_lowe_ratio", "surf_lowe_ratio", "cap_from_seeds"):
                raise TypeError(f"guided_match: unknown option {k}")
            setattr(o, k, int(v) if k == "cap_from_seeds" else v)
        Fin = None if F is None else np.ascontiguousarray(F, dtype=np.float64).reshape(n, 9)
        if capacity is None:
            capacity = sum(min(sum(self.view_size(a)), sum(self.view_size(b))) for a, b in flat.tolist())
        res = np.zeros(max(n, 1), dtype=_GUIDED_RESULT_DTYPE)
        corr = np.zeros((max(capacity, 1), 2), dtype=np.int32)
        Fout = np.zeros((max(n, 1), 9))
        total = C.c_int64()
        self.last_guided_total = None
        status = capi.lib.osfm_match_guided(self._h, flat.ctypes.data, n, off.ctypes.data, seeds.ctypes.data if seeds.size else None,
                                            Fin.ctypes.data if Fin is not None and Fin.size else None, C.byref(o), res.ctypes.data,
                                            corr.ctypes.data, C.c_int64(capacity), C.byref(total), Fout.ctypes.data)
        if status == capi.E_CAPACITY:
            self.last_guided_total = int(total.value)
        capi.check(status)
        return res[:n], corr[:int(total.value)], Fout[:n].reshape(n, 3, 3)

    def guided_arrays(self, pairs, records, corr, F=None, **options):
        """Guided matching of what compute_arrays returned: every OSFM_PAIR_MATCHED pair goes through osfm_match_guided
        with its list as seeds (F: None, or (n, 3, 3) with a row per pair of `pairs`).  Returns (records, corr, F_used):
        a copy of `records` whose counts (num_inliers with verification, else num_matches) and offsets describe the
        extended lists in the new corr, and the (n, 3, 3) F of every pair (zero where a pair was not guided).  The
        osfm_guided_result records of the guided pairs and their positions in `pairs` are left in self.last_guided."""
        flat = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        assert flat.shape[0] == len(records), "guided_arrays: records and pair list of different calls"
        cnt_field = "num_inliers" if self.opts.geometric_verification else "num_matches"
        sel = np.nonzero(records["status"] == capi.PAIR_MATCHED)[0]
        counts = records[cnt_field][sel].astype(np.int64)
        offs = np.zeros(sel.size + 1, np.int64)
        np.cumsum(counts, out=offs[1:])
        corr = np.asarray(corr).reshape(-1, 2)
        seeds = np.concatenate([corr[o:o + c] for o, c in zip(records["offset"][sel].tolist(), counts.tolist())] +
                               [np.zeros((0, 2), np.int32)]).astype(np.int32)
        Fsel = None if F is None else np.asarray(F, dtype=np.float64).reshape(-1, 3, 3)[sel]
        gres, gcorr, Fg = self.guided_match(flat[sel], offs, seeds, Fsel, **options)
        out = records.copy()
        out[cnt_field][sel] = gres["num_seeds"] + gres["num_added"]
        out["offset"][sel] = gres["offset"]
        Fused = np.zeros((flat.shape[0], 3, 3))
        Fused[sel] = Fg
        self.last_guided = (sel, gres)
        return out, gcorr, Fused

    def compute(self, pairs=None, capacity=None):
        """Matches `pairs` (default: all V(V-1)/2 pairs in the reference's
        triangular order, view_1 > view_2).  Returns one TwoViewMatching per
        input pair, in input order."""
        ra, corr = self.compute_arrays(pairs, capacity)
        return self.as_objects(ra, corr)

    def as_objects(self, ra, corr, pairs=None):
        """The TwoViewMatching list of what compute_arrays returned (pairs: the list that call
        was given; default: the most recent call's)."""
        flat = self._last_pairs_flat if pairs is None else np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        assert flat.shape[0] == len(ra), "as_objects: records and pair list of different calls"
        n = flat.shape[0]
        empty = np.zeros((0, 2), np.int32)
        verify = bool(self.opts.geometric_verification)
        # the result records as columns (one pass each) instead of 7 ctypes field reads per pair
        status, lowres = ra["status"].tolist(), ra["lowres_matches"].tolist()
        nm, ni, off = ra["num_matches"].tolist(), ra["num_inliers"].tolist(), ra["offset"].tolist()
        v1, v2 = flat[:, 0].tolist(), flat[:, 1].tolist()
        cnt = ni if verify else nm
        out = [TwoViewMatching(v1[k], v2[k],
                               corr[off[k]:off[k] + cnt[k]] if status[k] == capi.PAIR_MATCHED else empty,
                               status[k], lowres[k], nm[k], ni[k]) for k in range(n)]
        return out

    @staticmethod
    def ransac_fundamental(pos1, pos2, corr, max_iterations=1000, threshold=0.0015, seed=0, pair_id=0, device=0):
        """sfm::RansacFundamental::estimate for one pair; returns (count, inlier ids, F): the number of
        inliers (-1 below 8 matches), their ascending indices into corr and the 3x3 F of the winning hypothesis."""
        pos1 = np.ascontiguousarray(pos1, dtype=np.float32).reshape(-1, 2)
        pos2 = np.ascontiguousarray(pos2, dtype=np.float32).reshape(-1, 2)
        corr = np.ascontiguousarray(corr, dtype=np.int32).reshape(-1, 2)
        o = capi.RansacOptions(max_iterations, 0, threshold, seed)
        inl = np.zeros(max(corr.shape[0], 1), dtype=np.int32)
        n = C.c_int32()
        F = np.zeros(9)
        capi.check(capi.lib.osfm_ransac_fundamental(
            device, capi._ptr(pos1, C.c_float), pos1.shape[0], capi._ptr(pos2, C.c_float), pos2.shape[0],
            capi._ptr(corr, C.c_int32), corr.shape[0], C.byref(o), C.c_uint64(pair_id),
            capi._ptr(inl, C.c_int32), C.byref(n), capi._ptr(F, C.c_double)))
        return n.value, inl[:max(n.value, 0)].copy(), F.reshape(3, 3)

    @staticmethod
    def ransac_affine(pos1, pos2, corr, max_iterations=1000, threshold=0.0015, seed=0, pair_id=0, refit=True, device=0):
        """osfm_ransac_affine for one pair of orthographic views; returns (count, inlier ids, F, record): the number of
        inliers (-1 below 4 matches), their ascending indices into corr, the affine fundamental matrix in the 3x3 layout
        of ransac_fundamental's F, and a dict of the result record (best_iteration, ransac_inliers, refit_ran,
        refit_accepted)."""
        pos1 = np.ascontiguousarray(pos1, dtype=np.float32).reshape(-1, 2)
        pos2 = np.ascontiguousarray(pos2, dtype=np.float32).reshape(-1, 2)
        corr = np.ascontiguousarray(corr, dtype=np.int32).reshape(-1, 2)
        o = capi.RansacAffineOptions(max_iterations, 1 if refit else 0, threshold, seed)
        inl = np.zeros(max(corr.shape[0], 1), dtype=np.int32)
        n = C.c_int32()
        F = np.zeros(9)
        r = capi.RansacAffineResult(-1, 0, 0, 0)
        capi.check(capi.lib.osfm_ransac_affine(
            device, capi._ptr(pos1, C.c_float), pos1.shape[0], capi._ptr(pos2, C.c_float), pos2.shape[0],
            capi._ptr(corr, C.c_int32), corr.shape[0], C.byref(o), C.c_uint64(pair_id),
            capi._ptr(inl, C.c_int32), C.byref(n), capi._ptr(F, C.c_double), C.byref(r)))
        rec = {"best_iteration": r.best_iteration, "ransac_inliers": r.ransac_inliers,
               "refit_ran": r.refit_ran, "refit_accepted": r.refit_accepted}
        return n.value, inl[:max(n.value, 0)].copy(), F.reshape(3, 3), rec

    def use_result_buffer(self, buf):
        """Lets the caller provide the (rows, 2) int32 array compute() writes the match
        lists into, e.g. page-locked memory (orthosfm_amd.distributed.pinned_array)."""
        assert buf.dtype == np.int32 and buf.ndim == 2 and buf.shape[1] == 2 and buf.flags.c_contiguous
        self._corr_buf = buf

    def _take_buffer(self, rows):
        buf = getattr(self, "_corr_buf", None)
        if buf is None or buf.shape[0] < rows:
            buf = np.empty((rows, 2), dtype=np.int32)
            self._corr_buf = buf
        return buf[:rows]

    def cascade_hashes(self, view, type_=0):
        """CascadeHashing::LocalData of a view: (hashes (n, words) uint64, bucket ids (6, n) uint8)."""
        n = self.view_size(view)[type_]
        words = 2 if type_ == 0 else 1
        hashes = np.zeros((max(n, 1), words), np.uint64)
        ids = np.zeros((6, max(n, 1)), np.uint8)
        tmp = np.zeros(6 * max(n, 1), np.uint8)
        capi.check(capi.lib.osfm_match_get_cascade_hashes(self._h, view, type_, capi._ptr(hashes, C.c_uint64),
                                                          capi._ptr(tmp, C.c_uint8)))
        if n:
            ids = tmp[:6 * n].reshape(6, n)
        return hashes[:n], ids[:, :n]

    def stats(self) -> capi.MatchStats:
        s = capi.MatchStats()
        capi.check(capi.lib.osfm_match_get_stats(self._h, C.byref(s)))
        return s

    def shard_stats(self, shard: int) -> capi.MatchStats:
        """What one shard of a multi-device matcher did in the most recent call."""
        s = capi.MatchStats()
        capi.check(capi.lib.osfm_match_get_shard_stats(self._h, C.c_int(shard), C.byref(s)))
        return s

    def close(self):
        if self._h:
            capi.lib.osfm_match_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipCascadeHashing(HipExhaustiveMatching):
    """Drop-in for sfm::CascadeHashing (src/mve/sfm/cascade_hashing.h:29-221), the
    matcher the application selects (matching_mve.cpp:406-408): pairwise_match
    is the approximate cascade-hashing search, pairwise_match_lowres the
    exhaustive one it inherits."""

    def __init__(self, num_views: int, device: int = 0, options: capi.MatchOptions | None = None,
                 copy_results: bool = True):
        opts = options if options is not None else capi.default_match_options()
        opts.matcher_type = capi.MATCHER_CASCADE_HASHING
        super().__init__(num_views, device, opts, copy_results)
