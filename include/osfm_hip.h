/*
 * osfm_hip.h -- C ABI of the MI355X (gfx950) backend for OrthoSfM's hot path:
 *   (A) exhaustive pairwise descriptor matching  (src/mve/sfm, src/matching)
 *   (B) orthographic bundle adjustment           (src/bundle_adjustment, src/algorithms)
 *
 * Plain C: pointers, sizes, POD structs; no C++/torch types.  Every entry
 * point names the reference interface it replaces (paths relative to the
 * OrthoSfM source tree).  All functions return OSFM_OK (0) or a negative
 * osfm_status; osfm_last_error() returns a thread-local description.
 * The library never hands out memory the caller must free and never falls
 * back to a CPU implementation: without a usable gfx950 device every
 * compute entry point fails with OSFM_E_DEVICE.
 */
#ifndef OSFM_HIP_H
#define OSFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSFM_API __attribute__((visibility("default")))

typedef enum osfm_status {
    OSFM_OK = 0,
    OSFM_E_ARG = -1,       /* null / out-of-range argument (MVE throws std::invalid_argument) */
    OSFM_E_DEVICE = -2,    /* no HIP device / HIP runtime error */
    OSFM_E_RANGE = -3,     /* descriptor value outside the quantised range */
    OSFM_E_CAPACITY = -4,  /* caller buffer too small; required size reported */
    OSFM_E_STATE = -5,     /* call order violated (e.g. view not set) */
    OSFM_E_NUMERIC = -6,   /* BA: linear solve failed / non-finite values */
    OSFM_E_IO = -7         /* text formats: file cannot be opened / malformed line */
} osfm_status;

OSFM_API const char *osfm_last_error(void);
/* ABI version: OSFM_ABI_VERSION of the header the library was built from.  The library writes its public structs
 * (osfm_match_stats, osfm_ba_summary, ...) in full, so a caller built against another header must not run: the
 * adapters (the headers under orthosfm_amd/host) and the Python mirror compare this with their own OSFM_ABI_VERSION at load time.
 * 100: rounds 1-3; 101: osfm_ba_summary.flow_fallbacks, osfm_match_stats.surf_*; 102: one observation per camera
 * and point enforced, osfm_scene_set_cameras,
 * osfm_ba_summary.order_arcs / chain_blocks*.  New entries and new structs (the view front end, its marks) leave it alone:
 * nothing that a caller built against 102 reads or writes has changed.  osfm_match_options has since got
 * ransac_model / ransac_refit appended, and the library READS that struct: the three entries that take it are bound
 * under new symbol names by this header (see below it), and the symbols a caller built against the earlier header
 * binds keep the earlier, shorter layout.  Such a caller still runs correctly, so the version is still 102.  The
 * consensus filter (osfm_ba_consensus, osfm_scene_filter_consensus and their structs) is new entries only, and so
 * are the observation refinement (osfm_refine_* and its structs), the dense plane sweep (osfm_dense_*) and the
 * depth-map meshes (osfm_dense_set_map, osfm_dense_mesh_*, osfm_dense_download_mesh and their structs).  The
 * slanted-plane refinement (osfm_dense_refine_*, osfm_dense_download_refined and their structs) is new entries too;
 * osfm_dense_mesh_options.reserved, which the defaults set to 0, is now called refined_normals: same size, same offset,
 * and 0 is what it was. */
#define OSFM_ABI_VERSION 102
OSFM_API int osfm_version(void);
/* Number of visible HIP devices (0 when there is none). */
OSFM_API int osfm_device_count(void);
/* Free / total bytes of a device's HBM (hipMemGetInfo): lets a caller size its
 * batches and check that handles give their memory back. */
OSFM_API int osfm_device_memory(int device, uint64_t *free_bytes, uint64_t *total_bytes);

/* What the library itself holds in this process, by kind -- the counterpart of osfm_device_memory that does not
 * depend on what the HIP runtime keeps in pools of its own: after osfm_match_destroy of the last matcher
 * device_buffer_bytes, live_matchers are zero and pinned_host_bytes / live_streams / live_events are back at what
 * the per-process stream sets of the BA entries hold (they are kept for reuse); pool_cached_bytes is what
 * osfm_trim_device_memory would hand back. */
typedef struct osfm_memory_report {
    int64_t device_buffer_bytes;   /* grow-only device buffers owned by live handles (banks, scratch, hashes) */
    int64_t pool_live_bytes;       /* work arrays of calls in flight (BA, triangulation, filters) */
    int64_t pool_cached_bytes;     /* work arrays kept for the next call */
    int64_t pinned_host_bytes;     /* page-locked staging of live handles and of the kept stream sets */
    int32_t live_matchers;
    int32_t live_streams;
    int32_t live_events;
    int32_t reserved;
} osfm_memory_report;
OSFM_API int osfm_library_memory(osfm_memory_report *out);

/* The work arrays of the bundle-adjustment / triangulation / filter calls come from a
 * per-device cache of device memory (hipMalloc and hipFree cost 50-100 us apiece, dozens per
 * call, hundreds of calls per reconstruction); at most 8 GiB per device are kept.  This
 * hands what is cached on `device` (-1: all devices) back to the driver; *released_bytes
 * (may be NULL) reports how much that was. */
OSFM_API int osfm_trim_device_memory(int device, uint64_t *released_bytes);
/* Diagnostic: the one-launch Cholesky of osfm_ba_solve leaves 16 stamps per diagonal workgroup of
 * its most recent factorisation: stamps[161][32] (one row per block row), read by tools/chol_flow_trace.py (100 MHz
 * counter: start, L of the last column published, factor started, inverse published; shader
 * cycles of the pivot loop and of the factor; how the inverse arrived: 1 = sc1 copy, 2 =
 * same-XCD mailbox).  enable != 0 switches the recording on
 * (current device) and returns what was recorded so far; 0 returns it and switches it off. */
OSFM_API int osfm_ba_debug_chol_trace(int enable, int64_t *stamps);

/* Test hook: the number of polls a wait of the one-launch Cholesky makes before it gives the launch up
 * (<= 0: the default, 2^21).  A launch given up is repeated by osfm_ba_solve in the launch-per-column
 * form and counted in osfm_ba_summary.flow_fallbacks; set small, every wait that is not satisfied at
 * once takes that path. */
OSFM_API int osfm_ba_debug_flow_spin_limit(int limit);
/* Diagnostic (host code only, no device): the elimination order osfm_ba_solve would choose for a reduced camera
 * system (ba_order.hip) -- cam_ldim[C] unknowns per camera, pairs[num_pairs][2] the camera pairs that share a track.
 * cam_off[C]: the cameras' offsets in the order chosen (the natural ones when none is); blocks (may be NULL) [nblk + 1]
 * rows of 3 x 64 bits: bit k of row i = tile (i, k) of the factor exists; info[8] = { ordered (0 / 1), arcs K,
 * cameras per separator, unknowns incl. interior padding, blocks of 32, chain of dependent diagonal blocks in the
 * cameras' own order, chain in the order chosen, padding unknowns }.  blocks_capacity: rows `blocks` has room for. */
OSFM_API int osfm_ba_debug_order(int num_cameras, const int32_t *cam_ldim, int num_pairs, const int32_t *pairs,
    int32_t *cam_off, uint64_t *blocks, int blocks_capacity, int32_t *info);
/* Test hook (device 0): the dense Cholesky solve osfm_ba_solve runs on a reduced camera system of more than one block,
 * applied to num_systems given systems A[r] x[r] = b[r] of order n (A: [num_systems][n][n], only the lower triangle
 * is read; b, x: [num_systems][n]) one after the other on one stream, with ONE set of work arrays for the whole batch
 * as in the LM loop: hand-off flags zeroed once and a new epoch per system, the factor's matrix filled with NaN once
 * and never cleared.  n <= 32 is refused (those systems take a kernel of their own).
 * num_cameras > 0: cam_ldim[num_cameras] unknowns per camera (summing to n) and pairs[num_pairs][2], the cameras that
 * share a track: the elimination order osfm_ba_debug_order reports is looked for and, where one is chosen, the system
 * is laid out in it (interior padding rows, block pattern) and x comes back in the caller's order.
 * form 0: the form the solve would pick (the one-launch form where it fits), 1: launch per block column.  max_d /
 * max_groups > 0 (form 0 only): D workgroups / workgroups of the one-launch launch for this call, in place of the
 * defaults; OSFM_E_ARG when the one-launch form cannot run with them.  info[r]: the device's info word of system r
 * as it is -- 0, the position of a pivot that is not positive (> 0), or >= 2^20 for a launch given up (not repeated
 * here).  launch (may be NULL) [8] = { 1 one-launch form / 0 launch per column, its workgroups, D workgroups, P
 * workgroups, P tiles, arcs of the elimination order (0: natural order), unknowns laid out (padding included), blocks of 32 }. */
OSFM_API int osfm_ba_debug_cholesky_solve(int n, int num_systems, const double *A, const double *b, int num_cameras,
    const int32_t *cam_ldim, int num_pairs, const int32_t *pairs, int form, int max_d, int max_groups, double *x,
    int32_t *info, int32_t *launch);

/* Diagnostic of the RANSAC-F scoring loop.  Its Sampson tests are pre-classified in packed
 * single precision; a test only counts when the float result is out of reach of its error
 * bound, everything else is redone in the reference's double arithmetic, so the inlier
 * counts are the double ones (orthosfm_amd/csrc/ransac_kernels.hip).  mode 0: double path
 * only; 1: pre-classification (default); 2: pre-classification, every decision checked
 * against the double path on the device.  counters (may be NULL) receives what the
 * launches since the previous call counted in mode 2: [0] wrong decisions (must be 0),
 * [1] undecided tests, [2] tests.  Process-wide; not for concurrent use with matching. */
OSFM_API int osfm_ransac_selfcheck(int mode, uint64_t *counters);

/* ====================================================================== */
/* (A) Matching                                                            */
/* ====================================================================== */

/*
 * Tunables of sfm::MatchingBase::Options (src/mve/sfm/matching_base.h:25-31)
 * and sfm::bundler::Matching::Options (src/mve/sfm/bundler_matching.h:58-77),
 * with the values the application hard-codes
 * (src/matching/matching_mve.cpp:393-408).
 */
/* Matcher behind pairwise_match (bundler_matching.cc:31-41).  Cascade hashing
 * is sfm::CascadeHashing with its default Options (6 bucket groups of 2^8
 * buckets, 6..10 candidates, cascade_hashing.h:35-47); its hashes are computed
 * from ALL views (the descriptor average, cascade_hashing.cc:128-163), lazily
 * at the first match call after a view was set.  pairwise_match_lowres stays
 * exhaustive in both (CascadeHashing inherits it). */
#define OSFM_MATCHER_EXHAUSTIVE 0
#define OSFM_MATCHER_CASCADE_HASHING 1
/* Model of the geometric verification (osfm_match_options.ransac_model).  FUNDAMENTAL: the reference's RansacFundamental
 * (8-point samples, a general fundamental matrix).  AFFINE: the affine fundamental matrix of two orthographic views
 * (4-point samples, one least-squares refit), see osfm_ransac_affine. */
#define OSFM_RANSAC_FUNDAMENTAL 0
#define OSFM_RANSAC_AFFINE 1

typedef struct osfm_match_options {
    float sift_lowe_ratio;          /* 0.8f   matching_base.h:27 */
    float sift_distance_threshold;  /* FLT_MAX                    */
    float surf_lowe_ratio;          /* 0.7f   matching_base.h:29 */
    float surf_distance_threshold;  /* FLT_MAX                    */
    int32_t use_lowres_matching;    /* 1      matching_mve.cpp:400 */
    int32_t num_lowres_features;    /* 500    bundler_matching.h:68 */
    int32_t min_lowres_matches;     /* 5      bundler_matching.h:70 */
    int32_t min_feature_matches;    /* 50     matching_mve.cpp:403 */
    int32_t pairs_per_batch;        /* pairs resident in one launch group (0 = auto) */
    /* geometric verification (RansacFundamental, bundler_matching.cc:194-219) */
    int32_t geometric_verification; /* 0: osfm_match_all stops before RANSAC (default) */
    int32_t ransac_max_iterations;  /* 1000   ransac_fundamental.h:42 */
    double ransac_threshold;        /* 0.0015 matching_mve.cpp:395 */
    int32_t min_matching_inliers;   /* 30     matching_mve.cpp:402 */
    int32_t matcher_type;      /* OSFM_MATCHER_EXHAUSTIVE (default) or OSFM_MATCHER_CASCADE_HASHING:
                                * bundler::Matching::MatcherType, bundler_matching.h:52-56 */
    uint64_t ransac_seed;           /* stream seed of the counter-based sampler */
    /* Cascade hashing only.  0 (default): the Result layout of sfm::CascadeHashing --
     * a descriptor type that EITHER view lacks contributes no entries at all
     * (CascadeHashing::oneway_match returns before sizing its list,
     * cascade_hashing.h:341-342, so combine_results sees empty lists and applies no
     * offset, matching.cc:74-86).  1: the exhaustive matcher's layout (the block of a
     * type view_1 has is always present, -1 filled): consistent combined indices. */
    int32_t cascade_keep_empty_blocks;
    /* SIFT descriptors with a byte > 127 ("special": MVE renormalises after the 0.2 clamp,
     * sift.cc:830-839, so a descriptor with its energy in a few bins holds bytes of 128-180)
     * do not fit the raw int8 operand of the correction-free score-tile kernel.  A view with
     * at most this many of them keeps all its other descriptors on that kernel and the
     * special ones are scored by a kernel of their own; a view with more takes the slower
     * per-view operand forms.  0: default (512, also the largest value taken); negative: always the
     * per-view forms.
     * Results are identical either way. */
    int32_t special_kernel_max;
    /* Model of the geometric verification: OSFM_RANSAC_FUNDAMENTAL (default) or OSFM_RANSAC_AFFINE; any other value
     * is OSFM_E_ARG at create.  Everything around the estimator (the max(8, min_matching_inliers) gate, the
     * statuses, the lists) is the same in both. */
    int32_t ransac_model;
    int32_t ransac_refit;           /* 1      affine model only: osfm_ransac_affine_options.refit */
} osfm_match_options;

/* The entries that take an osfm_match_options are bound as *_v2 symbols: the struct grew by ransac_model and
 * ransac_refit, and the library cannot tell a shorter struct from its caller.  The library keeps the symbols
 * osfm_match_options_default / osfm_match_create / osfm_match_create_multi for binaries built against the header
 * before that: they write and read the struct up to special_kernel_max and take the defaults for the rest. */
#define osfm_match_options_default osfm_match_options_default_v2
#define osfm_match_create osfm_match_create_v2
#define osfm_match_create_multi osfm_match_create_multi_v2

OSFM_API int osfm_match_options_default(osfm_match_options *opts);

typedef struct osfm_matcher osfm_matcher;

/* Replaces the construction of an sfm::MatchingBase implementation
 * (bundler::Matching::Matching, src/mve/sfm/bundler_matching.cc:27-42). */
OSFM_API int osfm_match_create(int device, int num_views,
    const osfm_match_options *opts, osfm_matcher **out);
OSFM_API int osfm_match_destroy(osfm_matcher *m);

/*
 * The same matcher over several devices of one node, for the single C++ process that
 * drives the reference (bundler::Matching::compute, src/mve/sfm/bundler_matching.cc:58-136):
 * one worker thread and stream set per entry of device_ids for the duration of a call,
 * the descriptor bank on every device, the pairs of osfm_match_all dealt by work (N1*N2,
 * longest first), concurrent osfm_match_pair[_lowres] callers spread round robin.  No
 * data-path exchange between the devices; results (records, list order, bytes) are those
 * of osfm_match_create on one device.  A device id may appear more than once (logical
 * shards on one device).  Every other osfm_match_* entry takes the returned handle.
 */
OSFM_API int osfm_match_create_multi(const int *device_ids, int num_devices, int num_views,
    const osfm_match_options *opts, osfm_matcher **out);
/* The device of every shard (one entry for a single-device matcher). */
OSFM_API int osfm_match_get_devices(const osfm_matcher *m, int32_t *device_ids, int capacity,
    int32_t *num_devices);

/*
 * Host quantisation of float descriptors, i.e. convert_descriptor of
 * ExhaustiveMatching::init_sift / init_surf
 * (src/mve/sfm/exhaustive_matching.cc:17-38, 76-112).
 */
OSFM_API int osfm_quantize_sift(const float *src, int n, uint16_t *dst);
OSFM_API int osfm_quantize_surf(const float *src, int n, int16_t *dst);

/*
 * MatchingBase::init for one view (src/mve/sfm/matching_base.h:40,
 * ExhaustiveMatching::init, exhaustive_matching.cc:55-74).  The _float
 * variant takes Sift::Descriptor::data / Surf::Descriptor::data rows and
 * quantises them like the reference; the plain variant takes the already
 * quantised 16-bit lanes (0..255 / -127..127 [-128 accepted]).  Data is
 * copied to the device; the caller keeps ownership of its buffers (the
 * reference frees the float descriptors right after init,
 * bundler_matching.cc:54-55): values are range-checked and copied to page-locked
 * memory before the call returns, the transfer and the conversion kernels are
 * queued on a stream of their own and not waited for.  A view may be set while
 * matching calls that do not name it are in flight (a matching call waits for
 * the uploads of the views it names); setting a view that a running call names
 * is the caller's error.
 */
OSFM_API int osfm_match_set_view(osfm_matcher *m, int view,
    const uint16_t *sift, int n_sift, const int16_t *surf, int n_surf);
OSFM_API int osfm_match_set_view_float(osfm_matcher *m, int view,
    const float *sift, int n_sift, const float *surf, int n_surf);
/* A caller that feeds osfm_match_all in batches of growing size (a pipeline whose first batches name the few views
 * that are up already) says how many pairs its largest call will hold: the work arrays -- 13 MB of column partials
 * per 20 000-feature pair -- are then sized for that call by the first one, instead of being freed and allocated
 * again at every size on the way (0.7 s of a 200-view job).  A hint: calls of any size stay valid.  0 clears it.
 * (No reference counterpart: bundler::Matching::compute allocates per pair, bundler_matching.cc:86-160.) */
OSFM_API int osfm_match_expect_pairs(osfm_matcher *m, int32_t pairs_per_call);
OSFM_API int osfm_match_view_size(const osfm_matcher *m, int view,
    int *n_sift, int *n_surf);

/* FeatureSet::positions of a view (src/mve/sfm/feature_set.h:66): n = n_sift +
 * n_surf normalised (x, y) float pairs in the combined feature index space.
 * Needed only for geometric verification. */
OSFM_API int osfm_match_set_positions(osfm_matcher *m, int view, const float *xy, int n);

/*
 * MatchingBase::pairwise_match (matching_base.h:43-44;
 * ExhaustiveMatching::pairwise_match, exhaustive_matching.cc:114-144):
 * two-way SIFT + SURF matching, cross-check, combine.  m12 must hold
 * n_sift+n_surf ints of view_1, m21 those of view_2; unsuccessful = -1.
 * len12/len21 receive the lengths the reference's Result vectors would
 * have (a descriptor type that view_1 lacks contributes an EMPTY list).
 * Thread-safe (the reference calls it from an OpenMP loop).
 */
OSFM_API int osfm_match_pair(osfm_matcher *m, int view_1, int view_2,
    int32_t *m12, int32_t *len12, int32_t *m21, int32_t *len21);

/* MatchingBase::pairwise_match_lowres (matching_base.h:51-52;
 * exhaustive_matching.cc:146-180). */
OSFM_API int osfm_match_pair_lowres(osfm_matcher *m, int view_1, int view_2,
    int num_features, int32_t *count);

/*
 * sfm::Matching::twoway_match<T> (src/mve/sfm/matching.h:148-159) on the
 * stored descriptors of one type (0 = SIFT/unsigned short, 1 = SURF/short),
 * optionally restricted to the first num_features descriptors of each view
 * (0 = all): the two one-way lists BEFORE remove_inconsistent_matches.
 * m12 holds n1 ints, m21 n2 ints.
 */
OSFM_API int osfm_match_twoway(osfm_matcher *m, int view_1, int view_2,
    int descriptor_type, int num_features, int32_t *m12, int32_t *m21);

typedef struct osfm_pair {
    int32_t view_1;
    int32_t view_2;
} osfm_pair;

enum {
    OSFM_PAIR_MATCHED = 0,          /* survived both gates */
    OSFM_PAIR_REJECTED_LOWRES = 1,  /* bundler_matching.cc:146-158 */
    OSFM_PAIR_REJECTED_COUNT = 2,   /* bundler_matching.cc:163-172 */
    OSFM_PAIR_SKIPPED_EMPTY = 3,    /* a view without features, :96-99 */
    OSFM_PAIR_REJECTED_INLIERS = 4  /* bundler_matching.cc:203-210 (verification on) */
};

typedef struct osfm_pair_result {
    int32_t status;          /* OSFM_PAIR_* */
    int32_t lowres_matches;  /* -1 when the low-res gate did not apply */
    int32_t num_matches;     /* count_consistent_matches of the full match */
    int32_t num_inliers;     /* RANSAC inliers (-1 when verification is off / not reached) */
    int64_t offset;          /* first correspondence in `corr` (pairs of ints) */
} osfm_pair_result;

/*
 * Batched form of bundler::Matching::compute up to (not including) the
 * RANSAC stage (src/mve/sfm/bundler_matching.cc:58-192): low-res gate,
 * pairwise_match, count_consistent_matches, threshold, and the ordered
 * (feature_1, feature_2) correspondence list of bundler_matching.cc:176-192.
 * Results are returned in INPUT order (deterministic, unlike the
 * reference's thread-completion order).  corr receives 2 ints per
 * correspondence; if more than `capacity` correspondences are produced the
 * call fails with OSFM_E_CAPACITY and *total holds the required count.
 * With opts.geometric_verification the call continues through RANSAC-F
 * (bundler_matching.cc:194-219): the list of a pair then holds its num_inliers
 * inlier correspondences (TwoViewMatching::matches) and pairs with fewer than
 * max(8, min_matching_inliers) inliers are OSFM_PAIR_REJECTED_INLIERS.  With
 * opts.ransac_model = OSFM_RANSAC_AFFINE the estimator is osfm_ransac_affine's
 * in the place of RANSAC-F; everything around it is the same.
 */
OSFM_API int osfm_match_all(osfm_matcher *m, const osfm_pair *pairs,
    int num_pairs, osfm_pair_result *results, int32_t *corr,
    int64_t capacity, int64_t *total);

/* (view_1 > view_2) of linear pair index i, bundler_matching.cc:92-93. */
OSFM_API int osfm_pair_from_index(int64_t index, int32_t *view_1, int32_t *view_2);

/* Statistics of the most recent osfm_match_all / osfm_match_pair call on
 * this matcher, for bench.py's live roofline: device time of the dominant
 * kernel (HIP events on the launch stream) and its launch count. */
typedef struct osfm_match_stats {
    double tile_kernel_ms;     /* sum over the full-matching launches of the score-tile kernel */
    int32_t tile_kernel_launches;
    int32_t exact_scan_queries;  /* queries re-done by the wrap-exact kernel */
    int64_t mac_count;           /* sum of n1*n2*D over those launches */
    int64_t algorithmic_bytes;   /* descriptors read once + results written */
    double lowres_kernel_ms;     /* same, launches of the low-res gate (limited variant) */
    int32_t lowres_kernel_launches;
    int32_t tile_workgroups;     /* workgroups of the full-matching tile launches: row blocks x column segments
                                  * (like every field here: of the most recent call, which starts from zero) */
    int64_t lowres_mac_count;
    double cashash_kernel_ms;    /* cascade hashing mode: candidate search + NN kernel */
    int32_t cashash_kernel_launches;
    int32_t special_kernel_launches;
    double special_kernel_ms;    /* special descriptors (a byte > 127) against the other view */
    /* sampled workgroups of the correction-free tile kernel: shader cycles and ticks of the 100 MHz
     * counter they took; cycles / ticks * 100 MHz = the clock the chip held under that kernel */
    double tile_shader_cycles;
    double tile_refclk_ticks;
    /* the SURF (D = 64) share of tile_kernel_ms / tile_kernel_launches / mac_count: a view that carries both
     * descriptor types (the application's FEATURE_ALL, matching_mve.cpp:333) runs one launch per type */
    double surf_tile_kernel_ms;
    int32_t surf_tile_kernel_launches;
    int32_t reserved2;
    int64_t surf_mac_count;
} osfm_match_stats;
OSFM_API int osfm_match_get_stats(const osfm_matcher *m, osfm_match_stats *out);
/* The same record of ONE shard of a multi-device matcher (osfm_match_create_multi; shard 0 of a single-device
 * one): what that device did in the most recent call -- the balance of the deal can be read off mac_count. */
OSFM_API int osfm_match_get_shard_stats(const osfm_matcher *m, int shard, osfm_match_stats *out);

/* CascadeHashing::LocalData of one view (cascade_hashing.h:146-168), computed on
 * demand: hashes [n][2] (SIFT, type 0) or [n][1] (SURF, type 1) 64-bit words,
 * bucket_ids [6][n] (ids < 256).  Either output may be NULL. */
OSFM_API int osfm_match_get_cascade_hashes(osfm_matcher *m, int view, int type,
    uint64_t *hashes, uint8_t *bucket_ids);

/* RansacFundamental::Options (src/mve/sfm/ransac_fundamental.h:33-54). */
typedef struct osfm_ransac_options {
    int32_t max_iterations;   /* 1000 */
    int32_t reserved;
    double threshold;         /* 0.0015 */
    uint64_t seed;
} osfm_ransac_options;
OSFM_API int osfm_ransac_options_default(osfm_ransac_options *o);

/* RansacFundamental::estimate for one pair (ransac_fundamental.cc:26-60):
 * pos1/pos2 normalised feature positions, corr k (feature_1, feature_2) pairs.
 * inliers receives ascending ids into corr (capacity k); *num_inliers = -1 for
 * k < 8 (the reference throws).  F (9 doubles, row major) may be NULL.  The
 * sample stream is (seed, pair_id): results do not depend on batching. */
OSFM_API int osfm_ransac_fundamental(int device, const float *pos1, int n1, const float *pos2, int n2,
    const int32_t *corr, int k, const osfm_ransac_options *opts, uint64_t pair_id,
    int32_t *inliers, int32_t *num_inliers, double *F);

/* Verification of a pair of ORTHOGRAPHIC views: RANSAC over affine fundamental matrices (no counterpart in the
 * reference).  Two orthographic views are related by x2^T F_A x1 = a x2 + b y2 + c x1 + d y1 + e = 0, F_A =
 * [0 0 a; 0 0 b; c d e]: 4 degrees of freedom, 4 matches per sample, and the Sampson distance that
 * osfm_ransac_fundamental thresholds is exact for it (its denominator is a^2 + b^2 + c^2 + d^2).  refit != 0: when the
 * winner has at least 5 inliers, F_A is fitted once more to all of them by least squares (smallest eigenvector of the
 * scatter of (x2, y2, x1, y1)); the refit replaces the winner when it has at least as many inliers. */
typedef struct osfm_ransac_affine_options {
    int32_t max_iterations;   /* 1000 */
    int32_t refit;            /* 1 */
    double threshold;         /* 0.0015 */
    uint64_t seed;
} osfm_ransac_affine_options;
OSFM_API int osfm_ransac_affine_options_default(osfm_ransac_affine_options *o);

typedef struct osfm_ransac_affine_result {
    int32_t best_iteration;   /* iteration of the winning sample (-1: no hypothesis had an inlier) */
    int32_t ransac_inliers;   /* its inlier count, before the refit */
    int32_t refit_ran;        /* 1: the refit was computed (refit != 0 and ransac_inliers >= 5) */
    int32_t refit_accepted;   /* 1: F and the inlier list are the refit's */
} osfm_ransac_affine_result;

/* Arguments as osfm_ransac_fundamental; *num_inliers = -1 for k < 4 (nothing else is written then).  F (may be NULL)
 * receives F_A as 9 doubles, row major, in the layout above, scaled to a^2 + b^2 + c^2 + d^2 = 1 (up to rounding
 * after a refit): whatever reads the F of osfm_ransac_fundamental can read it.  result may be NULL. */
OSFM_API int osfm_ransac_affine(int device, const float *pos1, int n1, const float *pos2, int n2,
    const int32_t *corr, int k, const osfm_ransac_affine_options *opts, uint64_t pair_id,
    int32_t *inliers, int32_t *num_inliers, double *F, osfm_ransac_affine_result *result);

/* Guided matching of verified pairs of ORTHOGRAPHIC views (no counterpart in the reference): the nearest-neighbour
 * search of osfm_match_pair once more, restricted to the band |a x2 + b y2 + c x1 + d y1 + e| < threshold * sqrt(s)
 * around the affine epipolar line of a pair whose F_A is known.  The ratio test against the whole other view throws
 * repeated structure away (second ~ best); inside the band there is usually one candidate left.  Per pair:
 *   F      row p of F when given ((a, b, c, d, e) = F[2], F[5], F[6], F[7], F[8]); else the least-squares F_A over all
 *          seeds of the pair, which is osfm_ransac_affine's refit with every seed an inlier.  F NULL and fewer than 5
 *          seeds: OSFM_GUIDED_TOO_FEW.  s = a^2 + b^2 + c^2 + d^2 not > 0 or a coefficient that is not finite:
 *          OSFM_GUIDED_DEGENERATE.  Either way the pair's list is its seeds as given.  F_out receives the F used.
 *   band   j of view_2 is a candidate of i of view_1, and i of j, when the match (i, j) passes osfm_ransac_affine's
 *          own inlier test for F at `threshold`.  A feature that occurs in a seed is neither a query nor a candidate.
 *   search per descriptor type (indices and offsets as osfm_match_pair), NearestNeighbor<T>::find over the candidate
 *          rows in ascending feature index -- 16-bit lane sums, >= comparisons, T-typed state from (0, 0), the
 *          reference's conversion to distances -- then the ratio test of matching.h:114-146 with the squared ratio
 *          (0 / 0 accepted).  A query without candidates has no match.
 *   cap    cap_from_seeds: per type, the largest converted distance of a seed's own descriptor product; a result with
 *          dist_1st above it is dropped, and a type without seeds adds nothing.  (A lone distractor in the band passes
 *          a ratio test that has no second candidate; the seeds say how far a true match can be.)
 *   list   (i, j) is added when i -> j and j -> i.  The list holds the seeds and the additions, ascending in
 *          feature_1; every feature occurs once at most.
 * OSFM_E_ARG (nothing written): a view without positions, a seed out of range, a feature twice in a pair's seeds, a
 * seed that joins a SIFT row to a SURF row, offsets that decrease, a threshold that is not > 0.  OSFM_E_CAPACITY with
 * *total set as osfm_match_all.  A pair's results do not depend on what else is in the call, and a call repeats to
 * the byte.  Only the bank and the positions are read, whatever the matcher type; a multi-device handle runs the
 * call on its first shard. */
typedef struct osfm_guided_options {
    double  threshold;         /* 0.0015: the band, in the unit and by the test of osfm_ransac_affine's threshold */
    float   sift_lowe_ratio;   /* 0.8f */
    float   surf_lowe_ratio;   /* 0.7f */
    int32_t cap_from_seeds;    /* 1 */
    int32_t reserved;
} osfm_guided_options;
OSFM_API int osfm_guided_options_default(osfm_guided_options *o);

enum { OSFM_GUIDED_OK = 0, OSFM_GUIDED_TOO_FEW = 1, OSFM_GUIDED_DEGENERATE = 2 };
typedef struct osfm_guided_result {
    int32_t status;            /* OSFM_GUIDED_* */
    int32_t num_seeds;
    int32_t num_added;         /* correspondences in the list that are not seeds */
    int32_t max_candidates;    /* largest candidate count of one query of this pair (both directions, both types) */
    int64_t offset;            /* first correspondence of the pair in corr */
} osfm_guided_result;

/* The kernel's own sizes: queries a workgroup carries, positions it stages at a time, candidates a query collects
 * before they are scored (what the tests place their cases around). */
OSFM_API int osfm_guided_limits(int32_t *queries_per_workgroup, int32_t *positions_per_chunk, int32_t *candidates_per_pass);

/* seed_offsets [num_pairs + 1] in correspondences; seed_corr (feature_1, feature_2) pairs; F NULL or [num_pairs][9] in
 * osfm_ransac_affine's layout; opts NULL: the defaults; F_out NULL or [num_pairs][9]. */
OSFM_API int osfm_match_guided(osfm_matcher *m, const osfm_pair *pairs, int num_pairs,
    const int64_t *seed_offsets, const int32_t *seed_corr, const double *F,
    const osfm_guided_options *opts, osfm_guided_result *results,
    int32_t *corr, int64_t capacity, int64_t *total, double *F_out);

/* ====================================================================== */
/* (B) Bundle adjustment                                                   */
/* ====================================================================== */

enum {
    OSFM_BA_MODEL_QUATERNION = 0,  /* solver 0: OrthoQuaternionCamera */
    OSFM_BA_MODEL_EULER = 1        /* solvers 1-3: OrthographicCamera */
};

/*
 * Flattened form of the arguments of orthosfm::runBundleAdjustment
 * (src/bundle_adjustment/bundle_adjustment.h:18-20): cameras and tracks
 * become structure-of-arrays.
 *
 * cam_params: num_cameras x 7 doubles.
 *   QUATERNION: (qx, qy, qz, qw, offsetX, offsetY, scale)  -- Eigen coeff
 *     order, OrthoQuaternionCamera.h:83-86
 *   EULER:      (phi, theta, roll, offsetX, offsetY, scale, unused)
 *     -- OrthographicCamera.h:122-127
 * cam_const: num_cameras x 7 bytes, non-zero = parameter block constant
 *   (camera fixed or per-block flag; OrthoQuaternionRecoAlgorithm.cpp:141-145,
 *   OrthographicReconstructionAlgorithm.cpp:170-176).  For QUATERNION the
 *   first byte covers the whole 4-vector rotation block.
 * points: num_points x 4 homogeneous (Track::m_point, track.h:103), in/out.
 * obs_*: one entry per residual block in the order of
 *   bundle_adjustment.cpp:103-123; obs_point MUST be non-decreasing
 *   (observations of a track are contiguous) and a point is observed AT MOST
 *   ONCE per camera (the reference's tracks hold one feature per view: a
 *   track with two is a conflict and dropped, bundler_tracks.cc:120-145) --
 *   a repeated (camera, point) is refused with OSFM_E_ARG.
 */
typedef struct osfm_ba_problem {
    int32_t model;
    int32_t num_cameras;
    int32_t num_points;
    int32_t num_observations;
    double *cam_params;
    const uint8_t *cam_const;
    const int32_t *img_width;
    const int32_t *img_height;
    double *points;
    const double *obs_xy;
    const int32_t *obs_camera;
    const int32_t *obs_point;
} osfm_ba_problem;

/* Solver settings of bundle_adjustment.cpp:61-64,126-133 plus the Ceres
 * defaults the reference leaves untouched. */
typedef struct osfm_ba_options {
    double huber_delta;               /* 1.0   HuberLoss(1.0) */
    double function_tolerance;        /* 1e-6  */
    double gradient_tolerance;        /* 1e-10 */
    double parameter_tolerance;       /* 1e-10 */
    int32_t max_num_iterations;       /* 100   */
    int32_t optimize_points;          /* runBundleAdjustment's optimizePoints */
    double initial_trust_region_radius;  /* 1e4  */
    double max_trust_region_radius;      /* 1e16 */
    double min_trust_region_radius;      /* 1e-32 */
    double min_relative_decrease;        /* 1e-3 */
    double min_lm_diagonal;              /* 1e-6 */
    double max_lm_diagonal;              /* 1e32 */
    int32_t jacobi_scaling;              /* 1 */
    int32_t max_consecutive_invalid_steps;  /* 5 */
    int32_t device;
    int32_t verbose;
    /* runBundleAdjustment's retriangulatePoints (bundle_adjustment.cpp:77-83): the points
     * are first replaced by the ray intersections of their observations under the given
     * cameras (triangulateOrthographicTracks with resetExistingPoints; a point with fewer
     * than two observations keeps its input value).  The reference does this on a filtered
     * copy of the tracks that it discards; whether to keep the returned points is the
     * caller's choice. */
    int32_t retriangulate_points;      /* 0 */
    /* Which form of the solve runs (this field was `reserved`, always 0: offset and struct size are unchanged).
     * 0: the general form.  1: the one-workgroup form (the whole solve in one launch of one workgroup) where the
     * problem has at most 8 cameras and at most auto_max_observations observations (osfm_ba_small_limits), else
     * the general form.  2: the one-workgroup form; OSFM_E_ARG with more than 8 cameras.  Any other value:
     * OSFM_E_ARG.  The two forms differ in the order of their sums only; each repeats to the bit. */
    int32_t small_form;                /* 0 */
} osfm_ba_options;

enum {
    OSFM_BA_CONVERGENCE_FUNCTION = 1,
    OSFM_BA_CONVERGENCE_GRADIENT = 2,
    OSFM_BA_CONVERGENCE_PARAMETER = 3,
    OSFM_BA_CONVERGENCE_TRUST_REGION = 4,
    OSFM_BA_NO_CONVERGENCE = 5,       /* max iterations */
    OSFM_BA_FAILURE = 6
};

typedef struct osfm_ba_summary {
    double initial_cost;
    double final_cost;
    int32_t num_iterations;           /* LM iterations incl. rejected, like Ceres' iteration count */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    int32_t termination;              /* OSFM_BA_* */
    double mean_point_change;         /* bundle_adjustment.cpp:150-160 printout */
    double max_point_change;
    double solve_ms;                  /* device+host wall time of the whole call */
    double point_pass_ms;             /* summed device time (HIP events) per kernel family */
    double pair_pass_ms;
    double cholesky_ms;
    double back_pass_ms;
    int32_t linearizations;           /* number of point/pair pass executions timed */
    int32_t num_pair_entries;         /* observation pairs in the Schur complement lists */
    double lm_loop_ms;                /* wall time of the LM iterations alone (host control included;
                                       * problem upload, pair lists and the first linearisation are not) */
    int32_t flow_fallbacks;           /* factorisations whose one-launch form gave its launch up (its workgroups
                                       * were not all resident: the device was shared) and that were repeated in
                                       * the launch-per-column form; the results do not depend on it */
    int32_t order_arcs;               /* 0: the reduced camera system was factored in the cameras' own order; K > 0: the
                                       * cameras form a ring / strip (every track spans a short run of views) and the
                                       * system was laid out as K arcs + K separators, factored side by side */
    int32_t chain_blocks_natural;     /* longest chain of dependent 32-unknown diagonal blocks in the cameras' order ... */
    int32_t chain_blocks;             /* ... and in the order used */
} osfm_ba_summary;

OSFM_API int osfm_ba_options_default(osfm_ba_options *opts);

/* The constants of the one-workgroup form (osfm_ba_options::small_form): the most cameras it takes, the tracks it
 * walks per round, and the most observations at which small_form == 1 picks it (0: never).  Any pointer may be
 * NULL. */
OSFM_API int osfm_ba_small_limits(int32_t *max_cameras, int32_t *track_chunk, int32_t *auto_max_observations);

/* ceres::Solve on the problem runBundleAdjustment builds
 * (bundle_adjustment.cpp:61-145): cam_params and points updated in place. */
OSFM_API int osfm_ba_solve(const osfm_ba_problem *p, const osfm_ba_options *o,
    osfm_ba_summary *s);

/* Test hook: what osfm_ba_solve's kernels computed in its first LM iteration, copied out of the solve itself.
 * The caller allocates every array; nc = the free camera columns summed over the cameras (their tangent columns in
 * the cameras' own order: rotation, then offX / offY / scale), M points, C cameras.  Every quantity is in the Jacobi-
 * scaled tangent space the solve works in.  Copied after the first linearisation (before any factorisation): */
typedef struct osfm_ba_lin_capture {
    double *scale_c, *diag_c;     /* [nc] Jacobi scales; LM diagonal: clamped diag(J^T J), unscaled by the radius */
    double *S;                    /* [nc][nc] reduced camera system, LM term included: lower triangle, zero above */
    double *rhs;                  /* [nc] its right-hand side Jc^T r - W V^-1 g */
    double *scale_p, *diag_p;     /* [3M] */
    double *vinv;                 /* [9M] (V_j + diag_p / radius)^-1 row-major */
    double *ge;                   /* [3M] Jp^T r summed over the point's observations */
    /* ... and after the first iteration's solve, camera update, back pass and decision: */
    double *y_c;                  /* [nc] solution of S y = rhs (the camera step is -y) */
    double *cand_cams;            /* [7C] candidate cameras */
    double *cand_points;          /* [4M] candidate points */
    int32_t nc;                   /* set by the caller: the nc its arrays are sized for (OSFM_E_ARG when the problem's
                                   * layout has another) */
    int32_t reserved;
    /* filled in by the call */
    double initial_cost, grad_max, radius;       /* after the first linearisation */
    double model_cost_change, cand_cost;     /* of the first step, as the decision read them */
    double relative_decrease;     /* (x_cost - cand_cost) / model_cost_change recomputed on the host from the device's
                                   * values (lm_decide_logic's formula): only `accepted` is the kernel's own decision */
    int32_t stopped;              /* the solve stopped before its first step (nothing after the first copy is set) */
    int32_t accepted;             /* the first step was accepted */
    int32_t flow_aborted;         /* the first factorisation's one-launch form gave its launch up */
    /* padding rows of the laid-out system (interior ones of an elimination order and the tail up to the block
     * size): their number, the smallest and largest diagonal entry and the largest |entry| elsewhere in their rows
     * and columns, right-hand side included */
    int32_t num_pad;
    double pad_diag_min, pad_diag_max, pad_off_max;
    /* the regime the solve took */
    int32_t win_num, win_over;    /* observation windows; of those, windows of more than 256 observations */
    int32_t small_lists;          /* pair lists from the scan of a handful of cameras (else the sort) */
    int32_t dense;                /* dense Schur product (else pair lists) */
    int32_t dense_splits;         /* its split over K (1: the product written into S in place; 0: no dense product) */
    int32_t num_pairs, pair_chunk, max_chunks, multi_chunk_pairs;
    int32_t order_arcs;           /* 0: the cameras' own order */
    int32_t span, N;              /* laid-out unknowns (padding included), rounded up to the block */
    int32_t small_solve;          /* N == 32: factorisation and candidate cameras in one launch */
    int32_t one_launch;           /* the first factorisation took the one-launch form (else launch per column) */
    int32_t post_fused, back_fused;   /* LM control in the pair / back pass tails (else launches of their own) */
} osfm_ba_lin_capture;
/* Runs osfm_ba_solve on p (cam_params / points are updated in place as that does) with the two copies into cap; the
 * solve's launches and their order are the same.  osfm_ba_solve itself copies nothing. */
OSFM_API int osfm_ba_debug_linearization(const osfm_ba_problem *p, const osfm_ba_options *o, osfm_ba_lin_capture *cap);

/* ---- covariances of the adjusted cameras and points (the counterpart of ceres::Covariance on the reference's problem,
 * which the reference never calls) ----
 *
 * One linearisation at the problem's cameras and points AS GIVEN (no step is taken, nothing is modified).  J is the
 * Jacobian of the Huber-corrected residuals (the rows the solve linearises: apply_loss_function = true) in the solve's
 * tangent space -- camera columns: the free tangent columns in the cameras' own order (rotation, then offX / offY /
 * scale; osfm_ba_lin_capture's layout), point columns: the three tangent columns of the homogeneous point.  The
 * cofactor matrix Q = (J^T J)^-1 is computed through the Schur complement S = U - sum_j W_j V_j^-1 W_j^T with NO
 * Levenberg-Marquardt diagonal.  The matrices are returned unscaled: multiplying by variance_factor is the caller's.
 *
 * Gauge.  With one camera constant and the scales constant (what the reference's reconstruction produces) J^T J
 * still has one null direction: a translation of the scene along that camera's viewing axis, which every other camera
 * absorbs in its offsets.  depth_gauge != 0: if some camera has every block constant, ONE further offset is treated
 * as constant for this call -- with c0 the first all-constant camera, of the cameras with both offsets free the one
 * whose viewing axis makes the largest angle with c0's (as lines: the smallest |cosine|; ties: the lowest index),
 * and of its two image axes the one with the larger component along c0's viewing axis (ties: X).  The choice is
 * reported as gauge_camera / gauge_axis (0: offX, 1: offY; -1 / -1: nothing held).  THE HELD COLUMN COUNTS AS
 * CONSTANT in cam_ldim, nc and every output.  depth_gauge == 0: the masks are used exactly as given.
 *
 * Rank.  After the factorisation of S the smallest relative pivot min_i L_ii^2 / S_ii (S_ii: S's own diagonal
 * before elimination) is compared with min_pivot_ratio: below it the call returns OSFM_E_NUMERIC with
 * rank_deficient = 1 and min_pivot_seen set, and writes no covariance.  The same ratio is applied to the pivots of
 * the 3 x 3 V_j of every point.
 *
 * A point is invalid (point_valid 0, covariance zero) when it has fewer than two observations, when |w| < 1e-12 |x|
 * (|x|: the 2-norm of the homogeneous 4-vector), or when V_j fails the pivot test (parallel rays).  An invalid point
 * is LEFT OUT of the system: every other output is what the problem without that track gives.
 * With optimize_points == 0, S = U, nothing is left out and the point outputs are not written.
 * At most OSFM_BA_COV_MAX_UNKNOWNS camera unknowns (the inverse works on three dense N x N arrays): beyond that
 * OSFM_E_CAPACITY. */
#define OSFM_BA_COV_MAX_UNKNOWNS 8192
typedef struct osfm_ba_cov_options {
    double huber_delta;           /* 1.0 */
    double min_pivot_ratio;       /* 1e-8 */
    int32_t optimize_points;      /* 1 */
    int32_t depth_gauge;          /* 1 */
    int32_t device;               /* 0 */
    int32_t reserved;
} osfm_ba_cov_options;

typedef struct osfm_ba_cov_result {
    /* set by the caller; any pointer may be NULL (that output is not written) */
    double *cam_cov;              /* [C][6][6] the camera's diagonal block of S^-1 in its first cam_ldim rows / columns, zero elsewhere */
    int32_t *cam_ldim;            /* [C] free tangent columns per camera (the held gauge column is not among them) */
    double *cam_cov_full;         /* [nc][nc] the whole S^-1, symmetric, cameras in the caller's order */
    double *point_cov;            /* [M][3][3] covariance of the Euclidean point (x/w, y/w, z/w): G (V_j^-1 + Y_j^T S^-1 Y_j) G^T */
    uint8_t *point_valid;         /* [M] */
    int32_t nc;                   /* the nc cam_cov_full is sized for (read when cam_cov_full != NULL: OSFM_E_ARG when
                                   * the problem's layout, gauge column held, has another; num_camera_unknowns and
                                   * the gauge fields then say what the layout has, nothing else is written) */
    int32_t reserved;
    /* filled in by the call */
    double cost;                  /* 1/2 sum rho over the observations of the system */
    double variance_factor;       /* 2 cost / (num_residuals - num_unknowns), 0 when that is not positive */
    double min_pivot_seen;        /* smallest relative pivot of S */
    int32_t num_residuals, num_unknowns;
    int32_t num_camera_unknowns;  /* nc */
    int32_t num_valid_points;
    int32_t gauge_camera, gauge_axis;
    int32_t rank_deficient;
    int32_t dense_schur;          /* the point part of S came from the dense product (dense visibility) */
    /* device time per kernel family (HIP events) and the wall time of the whole call */
    double linearize_ms, factor_ms, inverse_ms, point_ms, total_ms;
} osfm_ba_cov_result;

OSFM_API int osfm_ba_cov_options_default(osfm_ba_cov_options *opts);
/* The problem is validated as for osfm_ba_solve (a repeated (camera, point) is refused) and is not modified.
 * opts NULL: the defaults.  On OSFM_E_NUMERIC (rank deficient) the scalar fields are filled in, the arrays untouched. */
OSFM_API int osfm_ba_covariance(const osfm_ba_problem *p, const osfm_ba_cov_options *opts, osfm_ba_cov_result *res);

/* Batched ReconstructionAlgorithm::evaluateReprojectionError
 * (OrthoQuaternionRecoAlgorithm.cpp:175-194,
 * OrthographicReconstructionAlgorithm.cpp:204-223): err[k] = ||r_k||_2 in
 * pixels; residuals (2 per observation) may be NULL. */
OSFM_API int osfm_ba_reprojection_errors(const osfm_ba_problem *p, int device,
    double *err, double *residuals);

/* triangulateOrthographicTracks (src/triangulation/triangulation.cpp:44-93)
 * as called from runBundleAdjustment (bundle_adjustment.cpp:77-83):
 * points[j] = least-squares ray intersection over the track's observations,
 * point_valid[j] = 0 when fewer than two rays. */
OSFM_API int osfm_ba_triangulate(const osfm_ba_problem *p, int device,
    uint8_t *point_valid);

/* ---- outlier filters around the bundle adjustment ---- */

/* orthosfm::getNearestNeighbourDistance
 * (src/triangulation/outlier_filtering.cpp:14-38): nn[i] = min over j != i of
 * the 2-norm of the difference of the HOMOGENEOUS 4-vectors, 1000000 when no
 * point is closer.  points: [num_points][4]. */
OSFM_API int osfm_nn_distances(int device, const double *points, int32_t num_points,
    double *nn);

typedef struct osfm_outlier_stats {
    double mean;               /* of the nearest-neighbour distances */
    double sigma;              /* as the reference computes it (:80-98), after the 1e-3 floor */
    int32_t num_with_point;
    int32_t num_kept;
} osfm_outlier_stats;

/* orthosfm::filterOutlierTracks (outlier_filtering.cpp:40-125) on flattened
 * tracks: points [num_tracks][4] (Track::getPoint), has_point [num_tracks]
 * (Track::hasPoint); keep[t] = 1 when the track is in the returned list.
 * stats may be NULL. */
OSFM_API int osfm_filter_outlier_tracks(int device, const double *points,
    const uint8_t *has_point, int32_t num_tracks, uint8_t *keep,
    osfm_outlier_stats *stats);

/* ---- the incremental reconstruction's scene, resident on the device (the caller of path B) ----
 *
 * runPoseEstimation (src/sfm/reconstruct.cpp:193-281) hands filtered copies of its std::vector<Track> to every step:
 * per camera group filterTracksWithReprojectionError + a 3-camera runBundleAdjustment on a re-triangulated copy,
 * triangulateTracks over everything, every third group a global runBundleAdjustment, filterOutlierTracks and the
 * reprojection filter again.  Through the per-call entries above each of those calls flattens and uploads its
 * tracks.  A scene holds the track table ONCE -- features in track order, alive flags per feature and track, point
 * and hasPoint() per track, the aligned cameras -- and every step selects its observations from the flags on the
 * device.  What a filter of the reference drops from its list is a cleared flag here.  The per-call entries stay
 * (orthosfm_amd/host/ba_hip_adapter.h uses them); results are identical, step by step.  A scene is used by one
 * thread at a time (its entries lock it). */
typedef struct osfm_scene osfm_scene;

/* track_offsets [num_tracks + 1] (features of track t: [offsets[t], offsets[t+1])), feat_view / feat_xy per feature
 * (Feature::viewID and the float pixel position Feature::x / y, track.h:26-27), image size per view.  Every flag
 * starts alive, no track has a point, no view has a camera.  A track holds at most one feature per view (OSFM_E_ARG
 * otherwise; bundler_tracks.cc:120-145 drops such tracks). */
OSFM_API int osfm_scene_create(int device, int model, int num_views, const int32_t *img_width, const int32_t *img_height,
    int32_t num_tracks, const int64_t *track_offsets, const int32_t *feat_view, const float *feat_xy, osfm_scene **out);
OSFM_API int osfm_scene_destroy(osfm_scene *s);
/* alive flags from the caller's table (either may be NULL: unchanged).  Once the scene has dropped dead entries
 * (it compacts its table when enough have died) a flag that would set one of THOSE alive is refused with
 * OSFM_E_STATE and nothing changes: clearing flags always works. */
OSFM_API int osfm_scene_set_flags(osfm_scene *s, const uint8_t *alive_track, const uint8_t *alive_feature);
/* mergeIntoGlobal (reconstruct.cpp:236-247): the views get cameras (params [n][7], const masks [n][7] as in
 * osfm_ba_problem), appended to the aligned cameras in this order.  OSFM_E_STATE when a view has one already. */
OSFM_API int osfm_scene_align_views(osfm_scene *s, int n, const int32_t *views, const double *params, const uint8_t *cam_const);
/* Replaces the parameters (params [n][7]) of views that ARE aligned -- a caller's own change to alignedCameras, e.g.
 * normalizeScene when camera 0 is not the identity -- so that the device copy follows; OSFM_E_STATE for a view without
 * a camera.  The next osfm_scene_triangulate redoes every track, whatever new_views says. */
OSFM_API int osfm_scene_set_cameras(osfm_scene *s, int n, const int32_t *views, const double *params);
/* the aligned cameras in the order they joined (views / params may be NULL) */
OSFM_API int osfm_scene_get_cameras(osfm_scene *s, int capacity, int32_t *views, double *params, int32_t *num_cameras);
/* algorithm->triangulateTracks(alignedCameras, tracks, true) (triangulation.cpp:44-93): every alive track with two or
 * more rays under the aligned cameras gets its intersection, the other alive tracks lose their point (a dead track is
 * in no list of the reference: it keeps what it has in either kind of pass).  new_views != NULL: only
 * the tracks those views see are redone -- identical to the full pass as long as the other cameras have not moved
 * since the last one; check_full != 0 repeats the pass in full and counts the tracks that differ (*mismatches). */
OSFM_API int osfm_scene_triangulate(osfm_scene *s, int num_new_views, const int32_t *new_views, int check_full, int32_t *mismatches);
/* filterTracksWithReprojectionError(tracks, alignedCameras) (outlier_filtering.cpp:127-192), permanent */
OSFM_API int osfm_scene_filter_reprojection(osfm_scene *s, double max_error);
/* One camera group (reconstruct.cpp:205-219): the reprojection filter under the cameras (views, params, cam_const)
 * on a copy, then runBundleAdjustment(localCameras, localTracks, algorithm, true, true) on what it leaves -- the
 * tracks seen by at least two of the cameras, re-triangulated first, their points discarded afterwards.  params is
 * updated in place; the scene is not changed. */
OSFM_API int osfm_scene_local_adjustment(osfm_scene *s, int n, const int32_t *views, double *params, const uint8_t *cam_const,
    double max_error, const osfm_ba_options *opt, osfm_ba_summary *sum, int32_t *num_points, int32_t *num_observations);
/* runBundleAdjustment(alignedCameras, tracks, algorithm, true, false) (bundle_adjustment.cpp:49-161): every alive
 * track with a point, every live feature of it whose view has a camera; cameras and points updated in the scene. */
OSFM_API int osfm_scene_global_adjustment(osfm_scene *s, const osfm_ba_options *opt, osfm_ba_summary *sum, int32_t *num_points,
    int32_t *num_observations);
/* osfm_ba_covariance on exactly the selection osfm_scene_global_adjustment makes (alive tracks with a point, live
 * features of aligned views), bit for bit what the per-call entry gives on that problem.  Cameras in join order (C =
 * the aligned cameras); point_cov / point_valid per scene track in the caller's numbering ([num_tracks] as given to
 * osfm_scene_create; a track outside the selection is invalid, zero).  The scene is not changed. */
OSFM_API int osfm_scene_covariance(osfm_scene *s, const osfm_ba_cov_options *opts, osfm_ba_cov_result *res);
/* filterOutlierTracks over the alive tracks (outlier_filtering.cpp:40-125); what it drops loses its flag */
OSFM_API int osfm_scene_filter_outliers(osfm_scene *s, osfm_outlier_stats *stats, int32_t *num_killed);
/* the scene's state back: alive flags per track / feature, hasPoint() and point [num_tracks][4] (any may be NULL) */
OSFM_API int osfm_scene_download(osfm_scene *s, uint8_t *alive_track, uint8_t *alive_feature, uint8_t *has_point, double *points);


/* ---- initial alignment of a camera group: RANSAC over Tomasi-Kanade factorisations ----
 *
 * ReconstructionAlgorithm::calculateInitialAlignment (src/sfm/reconstruct.cpp:205):
 * robustlyEstimateTomasiKanadeFactorization (src/algorithms/tomasi_kanade.cpp:193-370) over the tracks every camera
 * of the group sees, then resolveAmbiguity (:372-444) between the two mirror solutions.  Deterministic: draw k of
 * iteration i of group g is the counter-based generator of the RANSAC-F above under (seed, g, i, k).  Where this
 * departs from the reference (closed-form metric upgrade, normalised coordinates, rotations as bases, the selection
 * rule, the fallback) and why: INTEGRATION.md section 3. */
typedef struct osfm_tk_options {
    int32_t sample_size;        /* 10     tracks per hypothesis, 4..32 (tomasi_kanade.cpp:208) */
    int32_t max_iterations;     /* 0      0: floor(log(1 - probability) / log(1 - inlier_ratio^sample_size)) = 241 (:212),
                                 *        held to 1 .. 2^20: at least one hypothesis runs (point 11);
                                 *        at most 2^20 may be asked for */
    double probability;         /* 0.999  :209 */
    double inlier_ratio;        /* 0.7    :210 */
    int32_t min_consensus;      /* 25     tracks outside the sample that must support a model (:221) */
    int32_t device;             /* 0 */
    double max_error_px;        /* 3.0    :222 */
    uint64_t seed;              /* 0      stream seed of the counter-based sampler */
} osfm_tk_options;
OSFM_API int osfm_tk_options_default(osfm_tk_options *opts);

enum {
    OSFM_TK_RANSAC = 0,         /* a supported model won */
    OSFM_TK_FALLBACK = 1,       /* no hypothesis had min_consensus: the factorisation of all given tracks (:361-365) */
    OSFM_TK_TOO_FEW = 2,        /* fewer than max(10, sample_size) tracks (the reference throws, :202-205) */
    OSFM_TK_DEGENERATE = 3      /* ... and the fallback's factorisation has no rank-3 / positive definite solution */
};

typedef struct osfm_tk_result {
    int32_t status;             /* OSFM_TK_* */
    int32_t iterations;         /* hypotheses drawn */
    int32_t usable_models;      /* ... that factorise and pass isTomasiKanadeResultUsable (:446-470) */
    int32_t supported_models;   /* ... and have min_consensus tracks */
    int32_t best_iteration;     /* the winner's iteration, -1 without one */
    int32_t num_inliers;        /* RANSAC: consensus + sample; FALLBACK: tracks within max_error_px in every camera */
    double mean_error_px;       /* mean reprojection error of those tracks over all cameras */
    double score_kernel_ms;     /* device time of the scoring kernel (all hypotheses x all tracks) */
} osfm_tk_result;

/* xy [num_tracks][num_cameras][2]: pixel positions, track-major, of tracks seen by every camera; 3 <= num_cameras <= 8.
 * basis_1 / basis_2 [num_cameras][9]: the two mirror solutions, one row-major rotation per camera (columns x, y, z
 * axis of the camera in the frame of camera 0, which is the identity); solution 1 is the one the hypotheses were
 * scored with.  offsets [num_cameras][2] (may be NULL): the cameras' offsets that put the world origin at the
 * centroid of the winning sample; inlier [num_tracks] (may be NULL).  opts NULL: the defaults. */
OSFM_API int osfm_tk_align(const double *xy, int32_t num_tracks, int32_t num_cameras, int32_t img_width, int32_t img_height,
    const osfm_tk_options *opts, uint64_t group_id, double *basis_1, double *basis_2, double *offsets, uint8_t *inlier,
    osfm_tk_result *result);
/* resolveAmbiguity, host only: global_rotation [num_cameras][9] row-major local -> world rotations of the group's
 * views that have a global camera (has_global[c] != 0; the others are not read).  With a and b the first two such
 * views, the difference of the look directions z_a - z_b in the frame where a is canonical is compared between the
 * global pair and each model by dot product: *choice = 1 or 2, the larger; ties or fewer than two shared views: 1. */
OSFM_API int osfm_tk_resolve_ambiguity(int32_t num_cameras, const double *basis_1, const double *basis_2,
    const double *global_rotation, const uint8_t *has_global, int32_t *choice);
/* osfm_tk_align on the scene's table: the live tracks seen by ALL n views (which need no cameras yet), in ascending
 * track order, cameras in the order of `views`; selected and gathered on the device.  The views must share one image
 * size.  *num_tracks (may be NULL): how many tracks that were; inlier (may be NULL) has capacity inlier_capacity and
 * is written for min(*num_tracks, inlier_capacity) of them. */
OSFM_API int osfm_scene_tk_align(osfm_scene *s, int n, const int32_t *views, const osfm_tk_options *opts, uint64_t group_id,
    double *basis_1, double *basis_2, double *offsets, uint8_t *inlier, int32_t inlier_capacity, osfm_tk_result *result,
    int32_t *num_tracks);


/* ---- placing one view against the scene's points: RANSAC over affine cameras (resection) ----
 *
 * The camera model is linear in the point: u = x.p / s - o_x, v = y.p / s - o_y in the normalised coordinates
 * u = -2 (px / W - 0.5), v = -2 (py / H - 0.5), so a view that sees N triangulated points is an affine camera
 * (u, v) = A X + (c, d) that four non-coplanar points fix.  Hypotheses from four-point samples (the sampler of the
 * entries above under (seed, stream_id, iteration, draw)), every hypothesis scored against all N points, the winner
 * refitted over its inliers and projected onto the camera model.  No mirror ambiguity (the points carry their
 * depth), no baseline enters, and no all-point fallback.  The reference has no such step; what is computed, in
 * full: INTEGRATION.md section 3b. */
typedef struct osfm_resect_options {
    int32_t max_iterations;     /* 0      0: floor(log(1 - probability) / log(1 - inlier_ratio^4)) = 107, held to 1 .. 2^20;
                                 *        at most 2^20 may be asked for */
    int32_t min_consensus;      /* 8      inliers outside the sample that must support a hypothesis */
    double probability;         /* 0.999 */
    double inlier_ratio;        /* 0.5 */
    double max_error_px;        /* 3.0    a point is an inlier iff its error is BELOW this (osfm_tk_options' value) */
    double min_pivot;           /* 1e-6   a sample is unusable when a pivot of its 3 x 3 elimination is below this times the
                                 *        largest entry of the matrix (coplanar or repeated points); the refit is refused when a
                                 *        pivot of its covariance is below this times the largest diagonal entry.  1e-6 keeps
                                 *        the rounding of either solve near 1e-10 and is far below what any sample that can
                                 *        gather support has */
    double min_axis_ratio;      /* 0.5    sigma_2 / sigma_1 of the hypothesis' 2 x 3 matrix below this: not a scaled-orthographic view */
    int32_t estimate_scale;     /* 0      != 0: scale = 2 / (sigma_1 + sigma_2) of the refitted matrix; 0: `scale` */
    int32_t device;             /* 0 */
    double scale;               /* 1.0    the camera's scale when it is not estimated (the reference's cameras: 1, fixed) */
    uint64_t seed;              /* 0      stream seed of the counter-based sampler */
} osfm_resect_options;
OSFM_API int osfm_resect_options_default(osfm_resect_options *opts);
/* points per scoring workgroup (the unit of the fixed-order sums) and hypotheses per staged chunk, as built
 * (either may be NULL) */
OSFM_API int osfm_resect_limits(int32_t *tile, int32_t *chunk);

enum {
    OSFM_RESECT_OK = 0,         /* a supported hypothesis won */
    OSFM_RESECT_TOO_FEW = 1,    /* n < 4 + min_consensus: nothing is launched */
    OSFM_RESECT_NO_MODEL = 2    /* no supported hypothesis: identity, scale opts.scale, zero offsets, no inliers */
};

typedef struct osfm_resect_result {
    int32_t status;             /* OSFM_RESECT_* */
    int32_t iterations;         /* hypotheses drawn */
    int32_t usable_models;      /* ... whose sample passes the pivot and axis-ratio tests */
    int32_t supported_models;   /* ... and have min_consensus inliers outside the sample */
    int32_t best_iteration;     /* the winner's iteration, -1 without one */
    int32_t ransac_inliers;     /* the winner's inliers under its own hypothesis (consensus + 4) */
    int32_t num_inliers;        /* inliers of the final camera */
    int32_t refit_used;         /* 1: the final camera comes from the refit over the winner's inliers; 0: from the winner */
    double mean_error_px;       /* mean error of the final camera's inliers */
    double score_kernel_ms;     /* device time of the scoring kernel (all hypotheses x all points) */
} osfm_resect_result;

/* points [n][3]: the points' positions; xy [n][2]: their pixel positions in the view (img_width x img_height).
 * rotation [9]: row-major local -> world (columns x, y, z axis, as osfm_tk_align's bases); *scale; offsets [2];
 * inlier [n] (may be NULL): the final camera's inliers.  opts NULL: the defaults.  stream_id: the sampler's stream
 * (osfm_tk_align's group_id). */
OSFM_API int osfm_resect_view(const double *points, const double *xy, int32_t n, int32_t img_width, int32_t img_height,
    const osfm_resect_options *opts, uint64_t stream_id, double *rotation, double *scale, double *offsets, uint8_t *inlier,
    osfm_resect_result *result);
/* osfm_resect_view on the scene's table: the live features of `view` (feature and track alive) whose track has a
 * point, in ascending feature order, X = point.xyz / point.w; selected and gathered on the device.  The view needs
 * no camera and the scene is not changed: the caller hands the result to osfm_scene_align_views.  *num_points (may
 * be NULL): how many correspondences that were; inlier (may be NULL) has capacity inlier_capacity and is written
 * for min(*num_points, inlier_capacity) of them. */
OSFM_API int osfm_scene_resect_view(osfm_scene *s, int32_t view, const osfm_resect_options *opts, uint64_t stream_id,
    double *rotation, double *scale, double *offsets, uint8_t *inlier, int32_t inlier_capacity, osfm_resect_result *result,
    int32_t *num_points);


/* The device part of orthosfm::filterTracksWithReprojectionError
 * (outlier_filtering.cpp:127-192).  p holds the FULL-SIZE tracks (the
 * caller's filterTracksToAvailableCameras(cameras, tracks, true, true)
 * selection, :131) flattened as for osfm_ba_solve.  They are re-triangulated
 * (triangulateTracks(cameras, fullSizeTracks, true), :134; p->points is
 * overwritten, point_valid[j] = 0 where fewer than two rays exist and the input
 * point is kept), every observation is evaluated against its track's point
 * (:158) and obs_keep[k] = err[k] < max_error (1.5 px in the reference, :140).
 * err and point_valid may be NULL. */
OSFM_API int osfm_filter_reprojection(const osfm_ba_problem *p, int device,
    double max_error, uint8_t *obs_keep, uint8_t *point_valid, double *err);

/* ---- per-track consensus triangulation: drop single wrong observations, keep the track ----
 *
 * Not in the reference, and opt-in.  filterTracksWithReprojectionError above intersects ALL rays of a track, the wrong
 * one included, and judges every feature against that pulled point; and it judges only tracks that every camera
 * sees.  Here every track of two or more observations is tested under the problem's cameras (DESIGN.md section 3.5b;
 * tests/consensus_restatement.py is the definition):
 *   sample     all n observations when n <= max_sample, else the observations floor(i n / max_sample)
 *   hypotheses every pair a < b of the sample, in lexicographic order: the midpoint of the common perpendicular of
 *              the two rays (skipped when 1 - (d_a . d_b)^2 <= 1e-12), scored against all n observations through
 *              the cameras' affine projections: inlier when the pixel distance is < max_error.  The winner has the
 *              most inliers, then the smallest sum of squared inlier errors, then the lowest index
 *   refit      refit_rounds times: the ray intersection of osfm_ba_triangulate over the mask, the errors of
 *              osfm_ba_reprojection_errors at it, the new mask err < max_error; a round that would fit fewer than two
 *              observations ends the loop.  refit_rounds == 0: the winner's midpoint and mask stand
 *   verdict    all n kept: CLEAN; at least min_support kept: REPAIRED; else UNSUPPORTED (every keep flag 0)
 * Tracks of fewer than two observations are UNTESTED, tracks without a valid pair DEGENERATE; both keep every
 * observation.  Results repeat to the bit and do not depend on the order of the tracks. */
enum {
    OSFM_CONSENSUS_UNTESTED = 0,
    OSFM_CONSENSUS_CLEAN = 1,
    OSFM_CONSENSUS_REPAIRED = 2,
    OSFM_CONSENSUS_UNSUPPORTED = 3,
    OSFM_CONSENSUS_DEGENERATE = 4
};
#define OSFM_CONSENSUS_MAX_REFIT_ROUNDS 16

typedef struct osfm_consensus_options {
    double max_error;             /* 1.5 px; > 0 */
    int32_t min_support;          /* 3; >= 2 */
    int32_t max_sample;           /* 16; 2..16 */
    int32_t refit_rounds;         /* 2; 0..OSFM_CONSENSUS_MAX_REFIT_ROUNDS */
    int32_t device;               /* osfm_ba_consensus only (a scene has its own) */
} osfm_consensus_options;
OSFM_API void osfm_consensus_options_default(osfm_consensus_options *opts);

/* how the kernels divide the work (tests place their sizes around these) */
typedef struct osfm_consensus_limits {
    int32_t short_length;         /* tracks of at most this many observations take the eight-lane path */
    int32_t short_tracks;         /* tracks per workgroup there */
    int32_t long_tracks;          /* tracks per workgroup of the wave-per-track path */
    int32_t max_sample;           /* the sample cap's upper limit */
} osfm_consensus_limits;
OSFM_API void osfm_consensus_get_limits(osfm_consensus_limits *limits);

typedef struct osfm_consensus_stats {
    int64_t tracks_tested;        /* two or more observations */
    int64_t tracks_clean, tracks_repaired, tracks_unsupported, tracks_degenerate;     /* sum: tracks_tested */
    int64_t tracks_unsettled;     /* the last two masks of the refit differ */
    int64_t obs_tested;           /* observations of the tested tracks */
    int64_t obs_dropped;          /* keep flags cleared */
    int64_t hypotheses_scored;    /* pairs that were not skipped */
    double device_ms;
} osfm_consensus_stats;

/* p as for osfm_ba_solve; nothing of it is written.  opts NULL: the defaults on device 0.  Every output may be NULL:
 * obs_keep [num_observations], track_status [num_points], points_out [num_points][4] (the consensus point of CLEAN and
 * REPAIRED tracks, the input point of every other), point_valid [num_points] (1: CLEAN or REPAIRED), obs_err
 * [num_observations] (the reprojection errors at points_out).  OSFM_E_ARG: a null problem or array, options out of
 * range. */
OSFM_API int osfm_ba_consensus(const osfm_ba_problem *p, const osfm_consensus_options *opts, uint8_t *obs_keep,
    int32_t *track_status, double *points_out, uint8_t *point_valid, double *obs_err, osfm_consensus_stats *stats);
/* The same over the scene's aligned cameras and every alive track with two or more live features in aligned views,
 * permanent: dropped features lose their flag; a track dies when its kept aligned features plus its live features in
 * views without a camera number fewer than two (the reference's newTrack.size() > 1); REPAIRED tracks that have a
 * point take the consensus point.  Everything else is untouched.  Equal, bit for bit, to osfm_ba_consensus on the
 * same features flattened in table order.  stats may be NULL. */
OSFM_API int osfm_scene_filter_consensus(osfm_scene *s, const osfm_consensus_options *opts, osfm_consensus_stats *stats);

/* ---- track building ---- */

typedef struct osfm_tracks_summary {
    int32_t num_tracks;           /* tracks in the output */
    int32_t num_invalid_tracks;   /* removed for holding two features of one view (bundler_tracks.cc:166-171) */
    int64_t num_features;         /* feature references in the output */
} osfm_tracks_summary;

/* sfm::bundler::Tracks::compute (src/mve/sfm/bundler_tracks.cc:49-145, with
 * unify_tracks :23-45 and remove_invalid_tracks :149-203) on flat arrays; host
 * code, like the reference's.
 *   view_sizes   [num_views]          features per view (positions.size())
 *   colors       [sum sizes][3]       FeatureSet::colors, views concatenated (NULL: black)
 *   pairs        [num_pairs]          TwoViewMatching::view_1_id / view_2_id, PairwiseMatching order
 *   pair_offsets [num_pairs + 1]      match range of each pair in corr (osfm_match_all's
 *                                     results give them: offset .. offset + num_inliers)
 *   corr         [..][2]              (feature in view_1, feature in view_2)
 * out:
 *   track_ids    [sum sizes]          Viewport::track_ids, views concatenated, -1 = none
 *   track_offsets[num_tracks + 1], track_features [..][2] = (view_id, feature_id)
 *                                     in the reference's order, track_colors [num_tracks][3]
 * Capacities count tracks / feature references; a safe bound for both is the
 * number of matches resp. twice that.  OSFM_E_CAPACITY leaves summary filled in. */
OSFM_API int osfm_tracks_compute(int32_t num_views, const int32_t *view_sizes,
    const uint8_t *colors, int32_t num_pairs, const osfm_pair *pairs,
    const int64_t *pair_offsets, const int32_t *corr, int32_t *track_ids,
    int64_t track_capacity, int64_t feature_capacity, int64_t *track_offsets,
    int32_t *track_features, uint8_t *track_colors, osfm_tracks_summary *summary);

/* The same with one explicit match range per pair: pair p owns
 * corr[pair_starts[p] .. pair_starts[p] + pair_counts[p]).  For match lists that
 * are not packed back to back -- the per-rank slices of a multi-GPU run lie in
 * one shared host segment (orthosfm_amd/distributed.py) and are consumed where
 * they are. */
OSFM_API int osfm_tracks_compute_ranges(int32_t num_views, const int32_t *view_sizes,
    const uint8_t *colors, int32_t num_pairs, const osfm_pair *pairs,
    const int64_t *pair_starts, const int64_t *pair_counts, const int32_t *corr,
    int32_t *track_ids, int64_t track_capacity, int64_t feature_capacity,
    int64_t *track_offsets, int32_t *track_features, uint8_t *track_colors,
    osfm_tracks_summary *summary);

/* Tracks::compute fed pair batch by pair batch (batches in the reference's pair order,
 * bundler_tracks.cc:66-119 is a sequential merge over the pairs): the host can merge the lists of
 * one batch of osfm_match_all while the device matches the next.  feed: pair p of the batch owns
 * corr[pair_starts[p] .. pair_starts[p] + pair_counts[p]) (2 ints per correspondence); finish
 * writes what osfm_tracks_compute writes (same arguments; track_ids may be NULL here) and leaves
 * the builder usable. */
typedef struct osfm_tracks_builder osfm_tracks_builder;
OSFM_API int osfm_tracks_builder_create(int32_t num_views, const int32_t *view_sizes, osfm_tracks_builder **out);
OSFM_API int osfm_tracks_builder_feed(osfm_tracks_builder *b, int32_t num_pairs, const osfm_pair *pairs,
    const int64_t *pair_starts, const int64_t *pair_counts, const int32_t *corr);
OSFM_API int osfm_tracks_builder_finish(const osfm_tracks_builder *b, const uint8_t *colors,
    int32_t *track_ids, int64_t track_capacity, int64_t feature_capacity,
    int64_t *track_offsets, int32_t *track_features, uint8_t *track_colors,
    osfm_tracks_summary *summary);
OSFM_API int osfm_tracks_builder_destroy(osfm_tracks_builder *b);

/* The feature table the reconstruction works on, from the tracks (the conversion at the end of
 * calculateTracksUsingMVE, matching_mve.cpp:455-466): for feature i of the tracks (track order,
 * track_features = (view, feature) pairs as osfm_tracks_compute writes them) view_out[i], feat_out[i],
 * xy_out[2i..] = the pixel position  float(image_width * (double(normalised) + 0.5))  for BOTH axes
 * (stored as the double of that float: Feature::x/y are float, track.h:26-27), track_of_out[i]
 * (may be NULL), and -- both or neither -- by_view_out (the feature indices grouped by view,
 * ascending inside a view) with view_start_out[num_views + 1].  norm_positions[v] points to view v's
 * [view_sizes[v]][2] normalised positions.  OSFM_E_RANGE for a feature outside its view. */
OSFM_API int osfm_tracks_feature_table(int64_t num_tracks, const int64_t *track_offsets,
    const int32_t *track_features, int32_t num_views, const int32_t *view_sizes,
    const float *const *norm_positions, double image_width,
    int32_t *view_out, int32_t *feat_out, double *xy_out, int32_t *track_of_out,
    int64_t *by_view_out, int64_t *view_start_out);

/* The observation arrays of an osfm_ba_problem from a scene's tracks in one pass -- what
 * runBundleAdjustment / triangulateOrthographicTracks build residual by residual from their
 * std::vector<Track> (bundle_adjustment.cpp:86-123, triangulation.cpp:43-93): features are in
 * track order; feature i is taken when live[i] != 0, camera_of_feature[i] >= 0 (its view has a
 * camera) and (track_mask == NULL or track_mask[track_of[i]] != 0).  obs_point[k] = track_slot[track]
 * when track_slot is given (the caller's numbering of the point blocks), else the rank of the track
 * among the tracks that contributed a feature -- their ids then go to tracks_out (capacity rows as
 * well).  feature_ids (may be NULL) receives the taken feature indices.  *num_observations is always
 * set; OSFM_E_CAPACITY when it exceeds `capacity`. */
OSFM_API int osfm_tracks_select_observations(int64_t num_features, const int32_t *track_of,
    const int64_t *track_offsets /* NULL, or the first feature of every track, [largest track id + 2] entries (features
                                    are in track order): the pass then goes track by track and jumps over unselected ones */,
    const int32_t *camera_of_feature, const uint8_t *live, const uint8_t *track_mask,
    const int32_t *track_slot, const double *xy, int64_t capacity, int32_t *feature_ids,
    double *obs_xy, int32_t *obs_camera, int32_t *obs_point, int32_t *tracks_out,
    int64_t *num_observations, int64_t *num_tracks_out);

/* orthosfm::buildGroups (src/data_structures/group.cpp:13-88, completeGroup
 * :90-155): the order in which the incremental reconstruction adds views, as
 * groups of group_size views (3 in the reference's algorithms).
 *   view_ids [num_views]   View::getID() in the order of the `views` vector
 *                          (views 0 and 1 seed the first group)
 *   tracks as CSR: track_offsets [num_tracks + 1], track_views [..] = Feature::viewID
 * out: groups [max_groups][group_size] view ids, group_tracks [max_groups]
 * (ViewGroup::tracks), *num_groups.  A score is the number of tracks holding
 * every view of the group (bitset popcounts on the device); candidates are taken
 * in ascending id order on ties, the first seed in lexicographic order among
 * seeds (the reference's OpenMP loop leaves ties to thread timing).
 * Precondition: no track holds a view twice (Tracks::remove_invalid_tracks has
 * run).  Such a track counts once for that view here, while the reference
 * counts features, so e.g. [1, 1, 2] is a full track of the group {1, 2, 4} to it.
 * OSFM_E_ARG (*num_groups untouched): null arrays, num_views < 2, duplicate ids,
 * group_size outside [3, 8].  OSFM_E_CAPACITY: more than max_groups groups; the
 * first max_groups are written.  OSFM_E_STATE, with the groups found until then
 * and their number in *num_groups:
 *   - a pick scores 0, i.e. a remaining view shares no track with any seed
 *     group.  The reference appends bestViewID's start value, view id 0, there:
 *     it goes on if id 0 is a view still unassigned (ids [4, 7, 0, 9] with
 *     tracks over 4, 7 and 9 only give it [4, 7, 9], [4, 7, 0] with 2 and 0
 *     tracks) and never terminates otherwise.  Here the call is refused in
 *     both cases.
 *   - num_views == 2, for which the reference returns the one group
 *     [v0, v1, 0] with 0 tracks.
 * OSFM_GROUPS_GENERAL in the environment (read on every call) sends group size
 * 3 down the general path of the other sizes instead of its incremental form. */
OSFM_API int osfm_build_groups(int device, int32_t num_views, const int32_t *view_ids,
    int32_t num_tracks, const int64_t *track_offsets, const int32_t *track_views,
    int32_t group_size, int32_t max_groups, int32_t *groups, int32_t *group_tracks,
    int32_t *num_groups);

/* ---------------------------------------------------------------------------
 * On-disk text formats of the pipeline either side of the path (SURVEY 8f rank
 * 4): what `orthosfm-app --calculated-tracks` reads and the testbench parses.
 * Host code.  Numbers are written by the same C++ stream operations the
 * reference uses (`ostream << float/double/unsigned`, `std::to_string(double)`),
 * so the bytes agree by construction.  Files that cannot be opened and lines
 * that do not parse give OSFM_E_IO (the reference's std::stoi/stod throw there).
 * ------------------------------------------------------------------------- */

/* orthosfm::Feature (src/data_structures/track.h:21-31), one record per track feature */
typedef struct osfm_track_feature {
    uint32_t view_id, local_feature_id, global_feature_id;
    float x, y;                   /* pixel coordinates */
    uint32_t r, g, b;
} osfm_track_feature;

/* saveTracksToFile (src/matching/matching_io.cpp:16-48): one line per track,
 * "count;view;local;global;x;y;r;g;b;view;..." -- tracks as CSR over features. */
OSFM_API int osfm_tracks_file_write(const char *path, int64_t num_tracks,
    const int64_t *track_offsets, const osfm_track_feature *features);

/* loadTracksFromFile (matching_io.cpp:50-97).  *num_tracks / *num_features are
 * always set to what the file holds; with capacities below that the call fails
 * with OSFM_E_CAPACITY and writes nothing else (call once with 0 capacities to
 * size the buffers).  track_offsets takes num_tracks + 1 entries. */
OSFM_API int osfm_tracks_file_read(const char *path, int64_t track_capacity,
    int64_t feature_capacity, int64_t *track_offsets, osfm_track_feature *features,
    int64_t *num_tracks, int64_t *num_features);

/* saveTracksToPairwiseFiles (matching_io.cpp:99-141): for every pair i < j of
 * view_ids the tracks reduced to exactly those two views
 * (filterTracksToAvailableCameras(ids, tracks, true, false), common.cpp:85-138),
 * one line "x_i y_i x_j y_j" each, in `folder`/%03d_%03d.txt; no file for a pair
 * without such tracks.  *files_written (may be NULL) counts the files. */
OSFM_API int osfm_tracks_pairwise_files_write(const char *folder, int32_t num_views,
    const uint32_t *view_ids, int64_t num_tracks, const int64_t *track_offsets,
    const osfm_track_feature *features, int64_t *files_written);

/* MVE tracks -> orthosfm tracks (src/matching/matching_mve.cpp:455-466):
 * feature (v, f) of an MVE track becomes Feature(v, f, 32768 v + f,
 * width (pos.x + 0.5), width (pos.y + 0.5)) -- the reference scales BOTH axes by
 * the image width -- with the feature's colour.
 *   track_features [num_features][2]  (view, feature), osfm_tracks_compute's output
 *   view_starts    [num_views + 1]    first row of each view in positions / colors
 *   positions      [..][2] float      FeatureSet::positions, views concatenated
 *   colors         [..][3]            FeatureSet::colors (NULL: 0) */
OSFM_API int osfm_tracks_from_mve(int64_t num_features, const int32_t *track_features,
    int32_t num_views, const int64_t *view_starts, const float *positions,
    const uint8_t *colors, double image_width, osfm_track_feature *features);

/* exportCamerasToFile / importCameraFileAsMatrix
 * (src/data_structures/camera_io.cpp:15-40, :42-71): "name;m00,m01,...,m33" with
 * the row-major 4x4 camera-to-world matrix [x y z origin; 0 0 0 1] in
 * std::to_string format.  Reading: names come back NUL-separated in names_buf;
 * *num_cameras / *names_bytes are always set, OSFM_E_CAPACITY as above. */
OSFM_API int osfm_cameras_file_write(const char *path, int32_t num_cameras,
    const char *const *image_names, const double *matrices);
OSFM_API int osfm_cameras_file_read(const char *path, int32_t camera_capacity,
    int64_t names_capacity, char *names_buf, double *matrices, int32_t *num_cameras,
    int64_t *names_bytes);

/* savePointsToPLY (src/util/common.cpp:141-188): ASCII PLY of the tracks that
 * have a point (has_point[t] != 0), xyz of the homogeneous point as written by
 * `ostream << double`, colour of the track's first feature. */
OSFM_API int osfm_sparse_cloud_write(const char *path, int64_t num_tracks,
    const int64_t *track_offsets, const osfm_track_feature *features,
    const double *points, const uint8_t *has_point);

/* saveRuntimesToTxt / runtimesFromTxt (src/util/timing.cpp:18-53); seconds[4] =
 * initialisation, track building, pose estimation, total. */
OSFM_API int osfm_time_measurements_write(const char *path, const double *seconds);
OSFM_API int osfm_time_measurements_read(const char *path, double *seconds);

/* ---------------------------------------------------------------------------
 * SIFT feature extraction (MVE's sfm/sift.cc and FeatureSet::compute_sift,
 * feature_set.cc:42-86), on the device.  The octave and DoG images, the candidate
 * list and the localised keypoints are equal to the reference's bytes; orientations
 * and descriptors are the same algorithm evaluated in double (DESIGN.md has the
 * measured distance).  This entry takes the image as the detector sees it; the
 * max_image_size halving loop of bundler_features.cc:66-68 is the view front end's
 * (last section).  SURF is the next section.
 * ------------------------------------------------------------------------- */
#define OSFM_SIFT_MAX_OCTAVES 16

/* Sift::Options and the capacity of a context's candidate and descriptor arrays. */
typedef struct osfm_sift_options {
    int32_t num_samples_per_octave;   /* 3 */
    int32_t min_octave;               /* 0, or -1: an octave of the doubled image first (values above 0 are refused) */
    int32_t max_octave;               /* 4 */
    float contrast_threshold;         /* negative: 0.02 / num_samples_per_octave */
    float edge_ratio_threshold;       /* 10 */
    float base_blur_sigma;            /* 1.6 */
    float inherent_blur_sigma;        /* 0.5 */
    int32_t max_keypoints;            /* 65536: more candidates than this is OSFM_E_CAPACITY (descriptors never exceed candidates) */
} osfm_sift_options;
OSFM_API int osfm_sift_options_default(osfm_sift_options *opts);

typedef struct osfm_sift_summary {
    int32_t num_candidates, num_keypoints, num_descriptors, num_octaves;
    int32_t keypoints_per_octave[OSFM_SIFT_MAX_OCTAVES];     /* entry 0 is octave min_octave */
    int32_t descriptors_per_octave[OSFM_SIFT_MAX_OCTAVES];
    /* stage times from events on the context's stream; localisation includes the keypoints' way to the host */
    double scale_space_ms, extrema_ms, localisation_ms, orientation_ms, descriptor_ms, total_ms;
} osfm_sift_summary;

typedef struct osfm_sift osfm_sift;

/* A context owns the pyramid and the work arrays for images up to max_width x max_height (booked in
 * osfm_library_memory as device_buffer_bytes) and serves one extraction at a time.  opts NULL: the defaults. */
OSFM_API int osfm_sift_create(int device, int max_width, int max_height, const osfm_sift_options *opts, osfm_sift **out);
OSFM_API int osfm_sift_destroy(osfm_sift *ctx);

/* Extracts the features of an 8-bit image in host memory, row-major, channels interleaved; 3 channels are
 * averaged (DESATURATE_AVERAGE).  On success the context holds the result until the next call and *summary
 * (may be NULL) is filled.  Errors, none of which writes *summary or leaves a result behind:
 *   OSFM_E_ARG       channels other than 1 or 3; a size on which the reference throws (create_octaves halves
 *                    the image once per octave, the last included, and halving needs 2 pixels a side)
 *   OSFM_E_RANGE     an image larger than the context
 *   OSFM_E_CAPACITY  more candidates than max_keypoints -- never a truncated result; a candidate yields one
 *                    keypoint and one descriptor at most, so neither of those can exceed it */
OSFM_API int osfm_sift_extract(osfm_sift *ctx, const uint8_t *pixels, int width, int height, int channels,
    osfm_sift_summary *summary);

/* The result of the last extraction in FeatureSet's order: by scale descending, descriptors of equal scale in
 * the order the detector generated them (the reference's std::sort leaves those unordered).  Every output is
 * caller-allocated for num_descriptors rows and may be NULL.
 *   descriptors [n][128], positions [n][2] (x, y in pixels of the input image), scale [n], orientation [n],
 *   colors [n][3] (linear_at on the byte image; a grey image gives its value three times),
 *   normalized_positions [n][2] (normalize_feature_positions with the principal point at 0.5, 0.5) */
OSFM_API int osfm_sift_download(osfm_sift *ctx, float *descriptors, float *positions, float *scale, float *orientation,
    uint8_t *colors, float *normalized_positions);

/* Test hooks.  osfm_sift_debug_image: image `index` of octave `octave` (min_octave .. max_octave) of the last
 * extraction; kind 0: the S + 3 octave images, kind 1: the S + 2 DoG images.  *width / *height (may be NULL)
 * are always set; out (may be NULL) takes width * height floats.
 * osfm_sift_debug_keypoints: rows (octave, sample, x, y) of the candidates (after_localisation 0) or of the
 * localised keypoints (1), in the detector's order; *count (may be NULL) is always set, out may be NULL. */
OSFM_API int osfm_sift_debug_image(osfm_sift *ctx, int octave, int kind, int index, float *out, int32_t *width,
    int32_t *height);
OSFM_API int osfm_sift_debug_keypoints(osfm_sift *ctx, int after_localisation, float *out, int32_t *count);

/* ---------------------------------------------------------------------------
 * SURF feature extraction (MVE's sfm/surf.cc and FeatureSet::compute_surf,
 * feature_set.cc:88-117), on the device.  Every stage -- the summed-area table, the
 * 4 x 4 response maps, candidates, localised keypoints, orientations, descriptors --
 * is held to the reference's bytes: float and double operations in its order, and
 * the values of expf, atan2, sinf and cosf taken from the host's C library.  The one
 * decision that cannot be pinned is the orientation window test of a sample whose
 * atan2f lies within a few ulps of a window bound (DESIGN.md 3u counts them).
 * This entry takes the image as the detector sees it; the halving loop is the view
 * front end's (last section).
 * ------------------------------------------------------------------------- */
#define OSFM_SURF_OCTAVES 4

/* Surf::Options and the capacity of a context's candidate and descriptor arrays. */
typedef struct osfm_surf_options {
    float contrast_threshold;         /* 500 */
    int32_t use_upright_descriptor;   /* 0 */
    int32_t max_keypoints;            /* 65536: more candidates than this is OSFM_E_CAPACITY (descriptors never exceed candidates) */
} osfm_surf_options;
OSFM_API int osfm_surf_options_default(osfm_surf_options *opts);

typedef struct osfm_surf_summary {
    int32_t num_candidates, num_keypoints, num_descriptors;
    /* descriptors with a sample tap outside the summed-area table, which the device reads as zero.  Always 0
     * for extracted features: the descriptor's margin 15 s + 1 holds every tap of a finite keypoint inside its
     * row.  The count is the guard of osfm_surf_debug_describe against non-finite input. */
    int32_t num_guarded;
    int32_t keypoints_per_octave[OSFM_SURF_OCTAVES];
    int32_t descriptors_per_octave[OSFM_SURF_OCTAVES];
    /* stage times from events on the context's stream; localisation, orientation and descriptors include their
     * results' way to the host */
    double sat_ms, response_ms, extrema_ms, localisation_ms, orientation_ms, descriptor_ms, total_ms;
} osfm_surf_summary;

typedef struct osfm_surf osfm_surf;

/* A context owns the summed-area table, the response maps and the work arrays for images up to
 * max_width x max_height (booked in osfm_library_memory as device_buffer_bytes) and serves one extraction at a
 * time.  opts NULL: the defaults. */
OSFM_API int osfm_surf_create(int device, int max_width, int max_height, const osfm_surf_options *opts, osfm_surf **out);
OSFM_API int osfm_surf_destroy(osfm_surf *ctx);

/* Extracts the features of an 8-bit image in host memory, row-major, channels interleaved; 3 channels are
 * desaturated on bytes (DESATURATE_LIGHTNESS).  No size is too small: an image that fits no filter has no
 * features, as in the reference.  On success the context holds the result until the next call and *summary (may
 * be NULL) is filled.  Errors, none of which writes *summary or leaves a result behind:
 *   OSFM_E_ARG       channels other than 1 or 3
 *   OSFM_E_RANGE     an image larger than the context
 *   OSFM_E_CAPACITY  more candidates than max_keypoints -- never a truncated result; a candidate yields one
 *                    keypoint and one descriptor at most, so neither of those can exceed it */
OSFM_API int osfm_surf_extract(osfm_surf *ctx, const uint8_t *pixels, int width, int height, int channels,
    osfm_surf_summary *summary);

/* The result of the last extraction in FeatureSet's order: by scale descending, descriptors of equal scale (SURF
 * has nine scales) in the order the detector generated them (the reference's std::sort leaves those unordered).
 * Every output is caller-allocated for num_descriptors rows and may be NULL.
 *   descriptors [n][64], positions [n][2], scale [n], orientation [n] (radians in [-pi, pi]), colors [n][3] and
 *   normalized_positions [n][2] as osfm_sift_download computes them */
OSFM_API int osfm_surf_download(osfm_surf *ctx, float *descriptors, float *positions, float *scale, float *orientation,
    uint8_t *colors, float *normalized_positions);

/* Test hooks.  osfm_surf_debug_image: response map `sample` (0..3) of octave `octave` (0..3) of the last
 * extraction; *width / *height (may be NULL) are always set; out (may be NULL) takes width * height floats.
 * osfm_surf_debug_keypoints: rows (octave, sample, x, y) of the candidates (after_localisation 0) or of the
 * localised keypoints (1), in the detector's order; *count (may be NULL) is always set, out may be NULL.
 * osfm_surf_debug_describe: Surf::descriptor_computation for one hand-placed descriptor on the last image's
 * summed-area table, scale in [1, 65) (else OSFM_E_ARG); *status 0: rejected (out is zero), 1: ok, 2: ok with taps
 * outside the table read as zero, which only non-finite x, y or orientation can bring about. */
OSFM_API int osfm_surf_debug_image(osfm_surf *ctx, int octave, int sample, float *out, int32_t *width, int32_t *height);
OSFM_API int osfm_surf_debug_keypoints(osfm_surf *ctx, int after_localisation, float *out, int32_t *count);
OSFM_API int osfm_surf_debug_describe(osfm_surf *ctx, float x, float y, float scale, float orientation, int upright,
    float *out, int32_t *status);

/* ---------------------------------------------------------------------------
 * View front end: bundler::Features::compute and the image part of calculateTracksUsingMVE
 * (matching_mve.cpp:144-152, bundler_features.cc:66-68) from a decoded byte image in host
 * memory to a view of a matcher.  One upload; the halving chain, both detectors, FeatureSet's
 * colours and normalised positions and the quantised bank of the matcher are made on the
 * device, and the float descriptors never cross the bus.  Image files, EXIF and .mve scenes
 * stay with the caller.
 * ------------------------------------------------------------------------- */
#define OSFM_FEATURE_SIFT 1
#define OSFM_FEATURE_SURF 2
#define OSFM_FEATURE_ALL 3

typedef struct osfm_view_options {
    int32_t downscale_factor;   /* 1: downscale_image runs downscale_factor - 1 halvings */
    int32_t max_image_size;     /* 6000000 (AppSettings); <= 0: no limit.  The image is halved while
                                   width * height > max_image_size, in int arithmetic as in the reference */
    int32_t feature_types;      /* OSFM_FEATURE_SIFT, OSFM_FEATURE_SURF or OSFM_FEATURE_ALL (the default) */
} osfm_view_options;
OSFM_API int osfm_view_options_default(osfm_view_options *opts);

typedef struct osfm_view_summary {
    int32_t import_width, import_height;      /* after downscale_factor: the reference's imageWidth */
    int32_t feature_width, feature_height;    /* after the max_image_size loop: what the detectors saw */
    int32_t num_halvings, num_sift, num_surf, reserved;
    osfm_sift_summary sift;                   /* zero where the detector did not run */
    osfm_surf_summary surf;
    /* device events: the halving chain, the colour and position kernel, and their sum with both detectors' total_ms */
    double halving_ms, view_ms, total_ms;
} osfm_view_summary;

typedef struct osfm_view_front osfm_view_front;

/* A front end owns two image buffers for inputs up to max_width x max_height x 3, a SIFT and a SURF context (per
 * feature_types) and the arrays of one view, all booked in osfm_library_memory.  The contexts are sized for the
 * largest image the chain can hand them: the input bound after the downscale_factor - 1 halvings, since an image
 * under max_image_size passes the loop as it is.  Any of the options may be NULL: the defaults. */
OSFM_API int osfm_view_front_create(int device, int max_width, int max_height, const osfm_view_options *view_opts,
    const osfm_sift_options *sift_opts, const osfm_surf_options *surf_opts, osfm_view_front **out);
OSFM_API int osfm_view_front_destroy(osfm_view_front *front);

/* Uploads an 8-bit image (row-major, channels interleaved, 1 or 3 channels), runs the halving chain
 * (mve::image::rescale_half_size<uint8_t>) and the detectors on its result, and computes colours and normalised
 * positions from the device image.  The result stays in the front end until the next call.  A call waits on the
 * device -- not on the host -- for an osfm_match_set_view_from_front that still reads the previous result.
 * Errors, none of which writes *summary or leaves a result behind:
 *   OSFM_E_ARG       channels other than 1 or 3; a size on which the reference throws: a halving of an image with a
 *                    side below 2, or an image the SIFT detector refuses (osfm_sift_extract)
 *   OSFM_E_RANGE     an image larger than max_width x max_height
 *   OSFM_E_CAPACITY  as osfm_sift_extract / osfm_surf_extract */
OSFM_API int osfm_view_front_load(osfm_view_front *front, const uint8_t *pixels, int width, int height, int channels,
    osfm_view_summary *summary);

/* The last load in FeatureSet's order, SIFT rows first then SURF rows, each by scale descending; every output is
 * caller-allocated and may be NULL.  With n = num_sift + num_surf:
 *   positions [n][2] (pixels of the feature image), normalized [n][2], colors [n][3], scale [n], orientation [n],
 *   sift_descriptors [num_sift][128], surf_descriptors [num_surf][64] */
OSFM_API int osfm_view_front_download(osfm_view_front *front, float *positions, float *normalized, uint8_t *colors, float *scale,
    float *orientation, float *sift_descriptors, float *surf_descriptors);

/* Test hook: the image the detectors saw; *width, *height, *channels (may be NULL) are always set, out (may be
 * NULL) takes width * height * channels bytes. */
OSFM_API int osfm_view_front_debug_image(osfm_view_front *front, uint8_t *out, int32_t *width, int32_t *height, int32_t *channels);

/* View masks and pixel colours: filterTracksWithMasks (src/matching/matching.cpp:325-368 with View::isPixelMaskedIn,
 * src/data_structures/view.cpp:100-112) and propagateColorsToTracks (src/util/common.cpp:289-315) as per-row lookups
 * at load time, while the import image is on the device.  Every row gets the pixel position the track conversion
 * will give it (pixel_width * (normalised + 0.5) on BOTH axes, osfm_tracks_from_mve's expression), a mark byte and
 * the colour of the import image's pixel under that position, truncated, not interpolated.
 *   mark bit 0 (OSFM_MARK_IN)       the row is masked in: mask value > threshold, or the view has no mask
 *   mark bit 1 (OSFM_MARK_OUTSIDE)  the reference's index lies outside the mask, where the reference reads past it;
 *                                   such a row counts as masked out
 * clamp OSFM_CLAMP_REFERENCE is the reference as written: x is clamped by rows - 1 and y by cols - 1, then the mask is
 * read at row y, column x.  OSFM_CLAMP_IMAGE clamps x by cols - 1 and y by rows - 1 and never leaves the mask.
 * The colour lookup clamps x by cols - 1 and y by rows - 1 of the import image, as the reference does.
 * mode OSFM_MARK_TRACKS leaves the load's result exactly that of osfm_view_front_load, the marks ride beside it (for
 * osfm_tracks_filter_marked).  OSFM_MARK_FEATURES removes the masked-out rows from the result: the summary's counts,
 * both downloads and osfm_match_set_view_from_front see the kept rows only, in their order -- byte for byte what
 * deleting those rows from a plain load's download gives.  That is not the reference (the ratio test sees fewer
 * candidates); it is the cheaper form for a caller who matches the masked object only. */
#define OSFM_MARK_TRACKS 0
#define OSFM_MARK_FEATURES 1
#define OSFM_CLAMP_REFERENCE 0
#define OSFM_CLAMP_IMAGE 1
#define OSFM_MARK_IN 1
#define OSFM_MARK_OUTSIDE 2

typedef struct osfm_view_mark_options {
    int32_t mode;          /* OSFM_MARK_TRACKS */
    int32_t clamp;         /* OSFM_CLAMP_REFERENCE */
    int32_t threshold;     /* 16: a row is masked in where the mask value is above it */
    int32_t pixel_width;   /* 0: this load's import_width -- the reference's imageWidth */
} osfm_view_mark_options;
OSFM_API int osfm_view_mark_options_default(osfm_view_mark_options *opts);

typedef struct osfm_view_mark_summary {
    int32_t masked_out_sift, masked_out_surf;   /* rows without OSFM_MARK_IN, per detector */
    int32_t outside;                            /* of those, rows with OSFM_MARK_OUTSIDE */
    int32_t kept_sift, kept_surf;               /* rows of the load's result (OSFM_MARK_TRACKS: every row) */
    int32_t has_mask, pixel_width, reserved;
} osfm_view_mark_summary;

/* osfm_view_front_load with the marks.  mask [mask_height][mask_width] bytes in host memory, at whatever size the
 * caller resized it to; NULL: a view without a mask (hasMask() false), which masks nothing.  opts NULL: the defaults.
 * *summary and *mark_summary may be NULL.  A chain with two or more max_image_size halvings would overwrite the import
 * image: the front end then takes a third image buffer (booked in osfm_library_memory), on the first such call.
 * Errors as osfm_view_front_load, and OSFM_E_ARG for a mask size that is not positive or options out of range. */
OSFM_API int osfm_view_front_load_marked(osfm_view_front *front, const uint8_t *pixels, int width, int height, int channels,
    const uint8_t *mask, int mask_width, int mask_height, const osfm_view_mark_options *opts, osfm_view_summary *summary,
    osfm_view_mark_summary *mark_summary);

/* The marks of the last osfm_view_front_load_marked, in the order of osfm_view_front_download (the kept rows with
 * OSFM_MARK_FEATURES); every output may be NULL: pixel_xy [n][2] float, pixel_rgb [n][3], mark [n].
 * OSFM_E_STATE after a plain osfm_view_front_load, or without a load. */
OSFM_API int osfm_view_front_download_marks(osfm_view_front *front, float *pixel_xy, uint8_t *pixel_rgb, uint8_t *mark);

/* Test hook, host code, no device needed: the row function the marks kernel runs, on host arrays.  normalized [n][2];
 * pixels is the import image; mask may be NULL; opts->mode is ignored and opts->pixel_width 0 means `width`. */
OSFM_API int osfm_view_debug_mark_rows(int64_t n, const float *normalized, const uint8_t *pixels, int width, int height,
    int channels, const uint8_t *mask, int mask_width, int mask_height, const osfm_view_mark_options *opts, float *pixel_xy,
    uint8_t *pixel_rgb, uint8_t *mark);

/* filterTracksWithMasks on tracks as CSR over (view, feature) -- osfm_tracks_compute's output -- and the marks of
 * every view, concatenated: view v's rows start at view_starts[v].  Host code.  keep[t] = 1 where every feature of
 * track t that lies in a view with a mask (view_has_mask[v] != 0) carries OSFM_MARK_IN; the marks of a view without
 * a mask are not read, and with no mask on any view every track is kept, as the reference returns its input.
 * *num_kept may be NULL.  OSFM_E_RANGE for a feature that names no row. */
OSFM_API int osfm_tracks_filter_marked(int64_t num_tracks, const int64_t *track_offsets, const int32_t *track_features,
    int32_t num_views, const int64_t *view_starts, const uint8_t *marks, const uint8_t *view_has_mask, uint8_t *keep,
    int64_t *num_kept);

/* Sets view `view` of the matcher from the front end's last load, on the device: what osfm_view_front_download ->
 * osfm_match_set_view_float -> osfm_match_set_positions (normalised, SIFT rows then SURF rows) would leave, byte for
 * byte.  As in osfm_match_set_view the work is queued on the matcher's upload stream, here behind an event of the
 * front end's stream, and the host waits only for two scalars (the number of special rows and the largest SURF
 * norm).  A multi-device matcher prepares the view on the first shard on the front end's device and copies the
 * prepared arrays to the others, device to device.
 *   OSFM_E_STATE  no load to hand off
 *   OSFM_E_ARG    the front end's device is none of the matcher's; a view id out of range
 * Neither touches the view. */
OSFM_API int osfm_match_set_view_from_front(osfm_matcher *m, int view, osfm_view_front *front);

/* Test hooks.  osfm_match_debug_view_bank: every array of a view that a matching call reads, in padded length.  The
 * counts are always set; each pointer may be NULL.  Lengths: sift, sift_raw [n_sift_pad][128]; sift_corr,
 * sift_raw_corr [n_sift_pad]; special [n_special_pad][128], special_corr [n_special_pad], special_map [n_special],
 * special_slot [n_sift] (the last four only where n_special > 0); surf [n_surf_pad][64], surf_corr [n_surf_pad];
 * positions [n_positions][2] (n_positions -1: never set).
 * osfm_match_debug_set_view_device: float rows in HOST memory and optional permutations (row i of the view is row
 * order[i]; NULL: the identity) are put on the device as they are and go through the device hand-off of
 * osfm_match_set_view_from_front, positions [n_sift + n_surf][2] included: values that no detector produces. */
typedef struct osfm_view_bank {
    int32_t n_sift, n_surf, n_sift_pad, n_surf_pad, n_special, n_special_pad, surf_norm2_max, n_positions;
    int8_t *sift, *sift_raw, *special, *surf;
    int32_t *sift_corr, *sift_raw_corr, *special_corr, *special_map, *special_slot, *surf_corr;
    float *positions;
} osfm_view_bank;
OSFM_API int osfm_match_debug_view_bank(osfm_matcher *m, int view, int shard, osfm_view_bank *bank);
OSFM_API int osfm_match_debug_set_view_device(osfm_matcher *m, int view, const float *sift, int n_sift, const int32_t *sift_order,
    const float *surf, int n_surf, const int32_t *surf_order, const float *positions);

/* ---- Sub-pixel refinement of track observations by affine least-squares patch matching -------------------------
 * No counterpart in the reference; a caller of it inserts the step behind calculateTracksUsingMVE.
 * tests/refine_restatement.py is the definition, DESIGN.md "Observation refinement" describes it.  In short: the first
 * alive observation of a track is its reference and never moves.  Its window T(u) = I_ref(p_ref + step u), u integer in
 * [-radius, radius]^2, sampled bilinearly, is the template of every other alive observation t of the track, which is
 * refined on its own: Gauss-Newton on T(u) ~ g I_t(p + A step u) + b over p (2), A (4), g and b, from the given
 * position, init_affine (or the identity), g = 1, b = 0, until |dp| < eps.  Pixel centres are at integers, as in
 * osfm_view_front_download's positions; a window is inside an image when every sample lies in [0, width - 1] x
 * [0, height - 1].  A 3-channel pixel has the grey value (float)(r + g + b) / 3.0f.  Everything from the samples on is
 * double arithmetic in a fixed order: a call repeats to the bit, and an observation's result does not depend on the
 * other tracks.
 *
 * One status per observation; out_xy is the input position, to the bit, for every status but OSFM_REFINE_REFINED.  The
 * first test that fails decides: */
#define OSFM_REFINE_UNTESTED 0          /* dead, or fewer than two alive observations in its track */
#define OSFM_REFINE_REFERENCE 1         /* the track's template */
#define OSFM_REFINE_REFINED 2
#define OSFM_REFINE_OUTSIDE 3           /* the template window, or the target window at any iteration or at the end, leaves its image */
#define OSFM_REFINE_FLAT 4              /* standard deviation of the template below min_contrast */
#define OSFM_REFINE_ILL_CONDITIONED 5   /* a pivot of the Cholesky factor of the diagonally scaled normal matrix below min_pivot */
#define OSFM_REFINE_NOT_CONVERGED 6     /* max_iterations steps without |dp| < eps */
#define OSFM_REFINE_REJECT_SHIFT 7      /* |p - p0| > max_shift */
#define OSFM_REFINE_REJECT_DEFORM 8     /* a singular value of A A0^-1 outside [1 / max_deform, max_deform] */
#define OSFM_REFINE_REJECT_SCORE 9      /* zero-mean normalised cross-correlation of the final patch and the template below min_score */
#define OSFM_REFINE_NUM_STATUS 10

typedef struct osfm_refine_options {
    int32_t radius;           /* 7: a 15 x 15 window; 2..15 */
    int32_t max_iterations;   /* 10; 1..100 */
    double step;              /* 1.0: pixels between neighbouring samples of the template; > 0 */
    double eps;               /* 1e-3 px */
    double min_contrast;      /* 2.0 grey levels */
    double max_shift;         /* 3.0 px */
    double max_deform;        /* 2.0; >= 1 */
    double min_score;         /* 0.9; -1..1 */
    double min_pivot;         /* 0.034 (how it was measured: DESIGN.md); 0 < min_pivot < 1 */
} osfm_refine_options;
OSFM_API int osfm_refine_options_default(osfm_refine_options *opts);

typedef struct osfm_refine_stats {
    int64_t status_count[OSFM_REFINE_NUM_STATUS];   /* observations per status */
    int64_t iterations;                             /* Gauss-Newton steps taken, summed */
    double device_ms;                               /* the two kernels, by device events */
} osfm_refine_stats;

typedef struct osfm_refiner osfm_refiner;

/* A refiner holds one grey image (float32, booked in osfm_library_memory as device_buffer_bytes) per view it was given. */
OSFM_API int osfm_refine_create(int device, int num_views, osfm_refiner **out);
OSFM_API int osfm_refine_destroy(osfm_refiner *r);
/* The image of a view, 8-bit, row-major, 1 or 3 interleaved channels, from host memory; the grey conversion runs on
 * the device.  OSFM_E_RANGE: view outside [0, num_views); OSFM_E_ARG: channels, a size outside 1..16384. */
OSFM_API int osfm_refine_set_image(osfm_refiner *r, int view, const uint8_t *pixels, int width, int height, int channels);
/* The same from the feature image of the front end's last load (what osfm_view_front_debug_image shows), device to
 * device, ordered against the front end's next load as osfm_match_set_view_from_front is.  OSFM_E_STATE without a
 * load; OSFM_E_ARG when the front end lives on another device. */
OSFM_API int osfm_refine_set_image_from_front(osfm_refiner *r, int view, osfm_view_front *front);

/* Tracks as CSR: observation f of track t for offsets[t] <= f < offsets[t + 1], F = offsets[num_tracks].  view [F],
 * xy [F][2] (pixels of the view's image), alive [F] (NULL: all alive), init_affine [F][4] row-major (NULL: identity),
 * opts NULL: the defaults.  Outputs, each [F] rows: out_xy [F][2], out_affine [F][4] (the refined A of REFINED
 * observations, the initial one of every other), score [F] (where the final patch was compared, else 0), status [F],
 * iterations [F]; out_affine, score, iterations and stats may be NULL.
 *   OSFM_E_ARG    null arguments, offsets that do not start at 0 or decrease, options out of range, a non-finite
 *                 position or init_affine, a singular init_affine
 *   OSFM_E_RANGE  a view id outside [0, num_views)
 *   OSFM_E_STATE  an alive observation in a view without an image
 * None of them writes an output. */
OSFM_API int osfm_refine_tracks(osfm_refiner *r, int64_t num_tracks, const int64_t *offsets, const int32_t *view, const double *xy,
    const uint8_t *alive, const double *init_affine, const osfm_refine_options *opts, double *out_xy, double *out_affine,
    double *score, int32_t *status, int32_t *iterations, osfm_refine_stats *stats);

/* ---- Dense depth maps by orthographic plane sweep, and their fusion into one point cloud -------------------------
 * No counterpart in the reference; a caller of it runs the step behind the last adjustment.
 * tests/dense_restatement.py is the definition, DESIGN.md "Dense plane sweep" describes it.  In short: every view v is
 * an affine camera, pixel = A_v X + t_v with P_v = [A_v | t_v] ([2][4] doubles, pixel centres at integers as in
 * osfm_view_front_download's positions).  A reference view r has the viewing axis d_r = (a0 x a1) / |a0 x a1| and
 * B_r = A_r^T (A_r A_r^T)^-1; its pixel x at depth z is the point X = B_r (x - t_r) + z d_r, seen in a source s at
 * (A_s B_r) x + (t_s - A_s B_r t_r) + z A_s d_r.  A sweep scores the depths z_k = z_min + k dz, k < num_depths: the
 * (2 radius + 1)^2 window of reference texels around x against the bilinear samples of the source at the warped
 * positions of the same pixels, by zero-mean normalised cross-correlation (float32 sums of the grey values minus
 * 128).  A source counts at a depth when every sample of the window lies in [0, width - 1] x [0, height - 1] and the
 * samples' variance is at least min_contrast^2; c[k] is the mean score over the sources that count, if there are
 * min_sources of them.  The best depth is the lowest k of the largest c[k], refined by the parabola through its two
 * neighbours.  One status per pixel; the first test that fails decides: */
#define OSFM_DENSE_OK 0
#define OSFM_DENSE_BORDER 1             /* the window leaves the reference image */
#define OSFM_DENSE_FLAT 2               /* variance of the reference window below min_contrast^2 */
#define OSFM_DENSE_NO_SOURCES 3         /* no depth at which min_sources sources count */
#define OSFM_DENSE_LOW_SCORE 4          /* the best c[k] below min_score */
#define OSFM_DENSE_RANGE_EDGE 5         /* the best k is 0 or num_depths - 1, or a neighbour of it has no c */
#define OSFM_DENSE_INCONSISTENT 6       /* osfm_dense_fuse: fewer than min_consistent other views agree */
#define OSFM_DENSE_DUPLICATE 7          /* osfm_dense_fuse: a view with a smaller index agrees and emits the point */
#define OSFM_DENSE_NUM_STATUS 8

typedef struct osfm_dense_options {
    int32_t radius;           /* 3: a 7 x 7 window; 1..7 */
    int32_t min_sources;      /* 2; 1..8 */
    int32_t min_consistent;   /* 2; >= 0 */
    int32_t reserved;
    double min_contrast;      /* 2.0 grey levels; > 0 */
    double min_score;         /* 0.8; -1..1 */
    double consistency_tol;   /* 2.0 depth steps of the supporting view; >= 0 */
} osfm_dense_options;
OSFM_API int osfm_dense_options_default(osfm_dense_options *opts);
/* The shape of the sweep kernel as built: the tile of reference pixels a workgroup owns, and the largest radius,
 * number of sources per sweep and number of depths it takes.  Any pointer may be NULL. */
OSFM_API int osfm_dense_limits(int32_t *tile_w, int32_t *tile_h, int32_t *max_radius, int32_t *max_sources, int32_t *max_depths);
/* Diagnostic of tools/dense_timing.py: the sweeps that follow (of every handle of the process) leave one part of the
 * kernel's work out, so that its share of the time shows -- 1: the texel gather, 2: the double arithmetic of the warped
 * positions (float32 instead), 3: all taps of the box sums but one; 0: the kernel as it is.  Their results mean
 * nothing.  Returns the mode that was set before. */
OSFM_API int osfm_dense_debug_ablation(int mode);

typedef struct osfm_dense_stats {
    int64_t status_count[OSFM_DENSE_NUM_STATUS];    /* pixels per status: of the swept view, or after a fusion of all swept views */
    int64_t samples;                                /* sweep: warped samples taken (halo texels x depths x sources) */
    double device_ms;                               /* the kernels, by device events */
} osfm_dense_stats;

typedef struct osfm_dense osfm_dense;

/* The handle holds one grey image per view (float32, as the refiner's), the cameras, and the depth map of every view
 * swept since the cameras were set: all booked in osfm_library_memory as device_buffer_bytes. */
OSFM_API int osfm_dense_create(int device, int num_views, osfm_dense **out);
OSFM_API int osfm_dense_destroy(osfm_dense *d);
/* The two setters of the refiner (osfm_refine_set_image, osfm_refine_set_image_from_front), same conversion, same
 * errors.  A new image drops the view's depth map. */
OSFM_API int osfm_dense_set_image(osfm_dense *d, int view, const uint8_t *pixels, int width, int height, int channels);
OSFM_API int osfm_dense_set_image_from_front(osfm_dense *d, int view, osfm_view_front *front);
/* P [num_views][2][4].  Clears all depth maps.  OSFM_E_ARG: a value that is not finite, or an A_v without rank 2. */
OSFM_API int osfm_dense_set_cameras(osfm_dense *d, const double *P);
/* The depth map of view ref against sources[num_sources] (1..max_sources other views, none twice).  opts NULL: the
 * defaults.  Outputs, each [height][width] of the view's image and each may be NULL: depth (NaN where the status is
 * not OSFM_DENSE_OK), score (c of the best depth; 0 there), status.  The map stays on the device for osfm_dense_fuse.
 * The result repeats to the bit and does not depend on what else was swept.
 *   OSFM_E_ARG    null handle or sources, options or num_depths (3..max_depths) out of range, dz <= 0 or values not
 *                 finite, num_sources outside 1..max_sources or below min_sources, a source equal to ref or repeated
 *   OSFM_E_RANGE  a view id outside [0, num_views)
 *   OSFM_E_STATE  no cameras, or ref or a source without an image
 * None of them writes an output. */
OSFM_API int osfm_dense_sweep(osfm_dense *d, int ref, int num_sources, const int32_t *sources, double z_min, double dz,
    int num_depths, const osfm_dense_options *opts, double *depth, float *score, uint8_t *status, osfm_dense_stats *stats);
/* Consistency and fusion over all views swept since the cameras were set.  An OK pixel of view r with point X looks, in
 * every other swept view s in ascending order, at the pixel nearest to A_s X + t_s: s supports it when that pixel is
 * inside and OK and its depth differs from d_s . X by at most consistency_tol steps of s.  Fewer than min_consistent
 * supporters: INCONSISTENT; else a supporter with a smaller index: DUPLICATE.  The cloud is what stays OK, in (view,
 * row, column) order; *num_points (may be NULL) is its size.  The sweeps' own results are not changed. */
OSFM_API int osfm_dense_fuse(osfm_dense *d, const osfm_dense_options *opts, int64_t *num_points, osfm_dense_stats *stats);
/* The status of a swept view after the last fusion, [height][width].  OSFM_E_STATE without one. */
OSFM_API int osfm_dense_download_status(osfm_dense *d, int view, uint8_t *status);
/* The cloud of the last fusion: points [N][3], view [N], pixel [N][2] (x, y); each may be NULL.  OSFM_E_STATE without a
 * fusion, OSFM_E_CAPACITY when capacity < N. */
OSFM_API int osfm_dense_download_cloud(osfm_dense *d, int64_t capacity, double *points, int32_t *view, int32_t *pixel);
/* Binary little-endian PLY: float x, y, z and uchar red, green, blue per vertex.  rgb [n][3] (NULL: zeros). */
OSFM_API int osfm_dense_cloud_write(const char *path, int64_t n, const double *points, const uint8_t *rgb);

/* ---- A mesh per depth map: islands, triangles, normals, scales, confidences ---------------------------------------
 * What MVE does between dmrecon and fssrecon (depthmap_cleanup, depthmap_triangulate, the vertex normals,
 * depthmap_mesh_confidences, the scale of scene2pset), on the image grid of an orthographic view; tests/mesh_restatement.py
 * is the definition, DESIGN.md "Depth-map meshes" describes it.  The footprint of a view is f = sqrt(|b0 x b1|) with b0,
 * b1 the columns of B: the side of a world square with a pixel's area.
 *
 * osfm_dense_set_map uploads a depth map in the layout osfm_dense_sweep returns ([height][width] each; score NULL:
 * zeros): the view then counts as swept -- an earlier fusion is gone, as after a sweep of it.
 *   OSFM_E_ARG    null handle, depth or status; a status above OSFM_DENSE_RANGE_EDGE; a depth that is not finite where
 *                 the status is OSFM_DENSE_OK; dz not finite or <= 0
 *   OSFM_E_RANGE  view outside [0, num_views)
 *   OSFM_E_STATE  no cameras, or the view has no image (which fixes the size)
 * None of them changes anything. */
OSFM_API int osfm_dense_set_map(osfm_dense *d, int view, const double *depth, const float *score, const uint8_t *status, double dz);

#define OSFM_MESH_VERTEX_SIMPLE 0       /* the incident triangles chain into a closed fan */
#define OSFM_MESH_VERTEX_BORDER 1       /* one open chain */
#define OSFM_MESH_VERTEX_COMPLEX 2      /* more than one chain */

typedef struct osfm_dense_mesh_options {
    double dd_factor;                   /* 5.0: an edge longer in depth than dd_factor footprints (sqrt 2 times that on a
                                         * diagonal) is a discontinuity and drops its triangles; 0: none is; >= 0 */
    int32_t confidence_iterations;      /* 3: confidence min(distance to the mesh border, K) / K; 0: all 1; 0..max */
    int32_t min_island;                 /* 0: 4-connected components of fewer solid pixels are cleared; >= 0 */
    int32_t use_fused;                  /* 0; 1: a pixel is solid only if the last fusion left it OK or DUPLICATE */
    int32_t refined_normals;            /* 0; not 0: a vertex whose pixel is OSFM_DENSE_REFINE_REFINED takes the normal of
                                         * osfm_dense_refine_view; every other vertex, and everything else, as with 0 */
} osfm_dense_mesh_options;
OSFM_API int osfm_dense_mesh_options_default(osfm_dense_mesh_options *opts);
/* The shape of the kernels as built: the tile of the component labelling, the largest confidence_iterations.  Any
 * pointer may be NULL. */
OSFM_API int osfm_dense_mesh_limits(int32_t *label_tile_w, int32_t *label_tile_h, int32_t *max_confidence_iterations);

#define OSFM_MESH_NUM_STAGES 5          /* labelling, triangles, vertices, confidence, scans and emission */
typedef struct osfm_dense_mesh_stats {
    int64_t pixels_solid;               /* before the islands are cleared */
    int64_t pixels_island;              /* cleared as islands */
    int64_t components;                 /* 4-connected components of the solid pixels (0 with min_island 0: no labelling) */
    int64_t triangles_dropped;          /* candidate triangles with a discontinuity on an edge */
    int64_t vertices_simple, vertices_border, vertices_complex;
    double threshold_steps;             /* dd_factor f / dz: the straight-edge threshold in depth steps of the view */
    double device_ms;                   /* all kernels, by device events */
    double stage_ms[OSFM_MESH_NUM_STAGES];
} osfm_dense_mesh_stats;

/* The mesh of one view's depth map (opts NULL: the defaults); it stays on the device until the next call, or until the
 * cameras, the view's image or the view's map change.  Solid pixels are those with sweep status OSFM_DENSE_OK (and see
 * use_fused); every 2 x 2 block of pixels gives up to two triangles in MVE's vertex order, blocks row-major; vertices
 * are the pixels a triangle names, row-major.  Repeats to the bit.  num_vertices, num_triangles, stats may be NULL.
 *   OSFM_E_ARG      null handle; dd_factor negative or not finite, confidence_iterations outside 0..max, min_island < 0
 *   OSFM_E_RANGE    view outside [0, num_views)
 *   OSFM_E_STATE    the view has no depth map; use_fused without a fusion; refined_normals on a view whose map was not
 *                   refined (osfm_dense_refine_view)
 *   OSFM_E_NUMERIC  the labelling ran into its iteration bound (65536 steps of one walk: a defect, or a component that
 *                   winds through more tile-local pieces than that in one chain; reported instead of a hang): no mesh
 * None of them writes an output. */
OSFM_API int osfm_dense_mesh_view(osfm_dense *d, int view, const osfm_dense_mesh_options *opts, int64_t *num_vertices,
    int64_t *num_triangles, osfm_dense_mesh_stats *stats);
/* The mesh of the last osfm_dense_mesh_view: points [V][3], unit normals [V][3] (towards the camera), confidence [V],
 * scale [V] (mean length of the mesh edges at the vertex), pixel [V][2] (x, y), vclass [V] (OSFM_MESH_VERTEX_*),
 * triangles [T][3] (vertex indices); each may be NULL.  OSFM_E_STATE without a mesh, OSFM_E_CAPACITY when
 * capacity_vertices < V or capacity_triangles < T. */
OSFM_API int osfm_dense_download_mesh(osfm_dense *d, int64_t capacity_vertices, int64_t capacity_triangles, double *points,
    double *normals, float *confidence, double *scale, int32_t *pixel, uint8_t *vclass, int32_t *triangles);
/* Binary little-endian PLY with MVE's property names: float x, y, z, nx, ny, nz, uchar red, green, blue, float
 * confidence, value (the scale) per vertex; faces as "list uchar int vertex_indices", left out with num_triangles 0
 * (a point set, as fssrecon reads it).  NULL: normals zeros, rgb zeros, confidence ones, scale zeros. */
OSFM_API int osfm_dense_mesh_write(const char *path, int64_t num_vertices, const double *points, const double *normals,
    const uint8_t *rgb, const float *confidence, const double *scale, int64_t num_triangles, const int32_t *triangles);

/* ---- Slanted-plane refinement of a depth map: sub-step depth, a depth gradient and a normal per pixel ---------------
 * An opt-in stage between sweep and fusion; tests/dense_refine_restatement.py is the definition, DESIGN.md
 * "Slanted-plane refinement" describes it.  Every OSFM_DENSE_OK pixel x of the view's map, at depth z0, gets the local
 * depth model z(x + u) = z + zx ux + zy uy.  With G = A_s B_r, g = t_s - G t_r, e = A_s d_r its window lands in source
 * s at (G x + g + z e) + (G + e (zx, zy)) u: one affine map per pixel and source, exact for a planar patch.
 * Gauss-Newton runs over (z, zx, zy), shared by the sources, and a gain and a bias per source, on the residuals
 * gain_s W_s(u) + bias_s - T(u): T the reference window (grey values, u integer in [-radius, radius]^2), W_s the
 * bilinear samples of source s.  A source counts when every sample of its window at (z0, 0, 0) lies in
 * [0, width - 1] x [0, height - 1]; the set is fixed there.  From the samples on everything is double arithmetic in a
 * fixed order: a call repeats to the bit and a pixel's result does not depend on any other pixel.
 *
 * One status per pixel; the first test that fails, in time, decides: */
#define OSFM_DENSE_REFINE_NOT_OK 0          /* the sweep's status is not OSFM_DENSE_OK: untouched */
#define OSFM_DENSE_REFINE_REFINED 1
#define OSFM_DENSE_REFINE_OUTSIDE 2         /* the reference window leaves its image; fewer than min_sources sources count; a
                                             * counting source's window leaves its image at an iteration or at the end */
#define OSFM_DENSE_REFINE_ILL_CONDITIONED 3 /* the gain/bias block of a source is singular, or a pivot of the Cholesky factor
                                             * of the diagonally scaled 3 x 3 normal matrix is below min_pivot */
#define OSFM_DENSE_REFINE_NOT_CONVERGED 4   /* max_iterations steps without |dz| <= eps dz and radius (|dzx| + |dzy|) <= eps dz */
#define OSFM_DENSE_REFINE_REJECT_SHIFT 5    /* |z - z0| > max_shift steps */
#define OSFM_DENSE_REFINE_REJECT_SLOPE 6    /* a singular value of a counting source's G + e (zx, zy) outside [1 / max_deform, max_deform] */
#define OSFM_DENSE_REFINE_REJECT_SCORE 7    /* the mean over the counting sources of the zero-mean normalised correlation of T
                                             * and W_s at the end is below min_score, or below what it was at the start */
#define OSFM_DENSE_REFINE_NUM_STATUS 8

typedef struct osfm_dense_refine_options {
    int32_t radius;           /* 3: the sweep's window; 1..7 */
    int32_t min_sources;      /* 2; 1..8 */
    int32_t max_iterations;   /* 10; 1..100 */
    int32_t reserved;
    double eps;               /* 1e-3 depth steps of the view; > 0 */
    double max_shift;         /* 1.5 depth steps: the sweep's best index is within one step of its own peak; >= 0 */
    double max_deform;        /* 2.0, as osfm_refine_options; >= 1 */
    double min_score;         /* 0.8, the sweep's; -1..1 */
    double min_pivot;         /* 0.035 (how it was measured: DESIGN.md); 0 < min_pivot < 1 */
} osfm_dense_refine_options;
OSFM_API int osfm_dense_refine_options_default(osfm_dense_refine_options *opts);

typedef struct osfm_dense_refine_stats {
    int64_t status_count[OSFM_DENSE_REFINE_NUM_STATUS];    /* pixels per status */
    int64_t iterations;                                     /* Gauss-Newton steps taken, summed */
    int64_t samples;                                        /* warped samples taken (window x source evaluations) */
    double device_ms;                                       /* the kernel, by device events */
} osfm_dense_refine_stats;

/* Refines the map of `view` (swept, or uploaded by osfm_dense_set_map) as it stands, against sources[num_sources]: the
 * pixels that come out REFINED take the new depth and, as their score, the mean correlation at the end; all others
 * keep the map's depth and score.  The handle keeps, per pixel, the status, the gradient (zx, zy) in depth per pixel
 * and the unit normal cross(b1 + zy d, b0 + zx d) / |.| (b0, b1 the columns of B_r; n . d < 0: towards the camera, the
 * sign of the meshes' vertex normals); gradient and normal are NaN where the status is not REFINED.  The sweep's own
 * status plane does not change, so the fusion and the meshes see the same solid pixels; the view still counts as
 * swept, and an earlier fusion and an earlier mesh of it are gone, as after a sweep.  Refining a view twice refines
 * the refined depths.  opts NULL: the defaults.  Outputs, each [height][width] rows of the view's image and each may be
 * NULL: depth, gradient [.][2], normal [.][3], score, rstatus -- the whole planes as they stand after the call.
 *   OSFM_E_ARG    null handle or sources, options out of range, num_sources outside 1..max_sources or below
 *                 min_sources, a source equal to view or repeated
 *   OSFM_E_RANGE  a view id outside [0, num_views)
 *   OSFM_E_STATE  no cameras, no map of the view, or a source without an image
 * None of them writes anything. */
OSFM_API int osfm_dense_refine_view(osfm_dense *d, int view, int num_sources, const int32_t *sources,
    const osfm_dense_refine_options *opts, double *depth, double *gradient, double *normal, float *score, uint8_t *rstatus,
    osfm_dense_refine_stats *stats);
/* What the last osfm_dense_refine_view of the view left on the device; each may be NULL.  OSFM_E_RANGE: the view;
 * OSFM_E_STATE: the view's map was not refined (a new image, new cameras or a new map drop the planes). */
OSFM_API int osfm_dense_download_refined(osfm_dense *d, int view, double *gradient, double *normal, uint8_t *rstatus);

#ifdef __cplusplus
}
#endif
#endif /* OSFM_HIP_H */
