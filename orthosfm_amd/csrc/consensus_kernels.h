// Per-track consensus triangulation: which observations of a track agree on one point.
//
// Every pair of (sampled) rays of a track proposes the midpoint of its common perpendicular; a proposal is scored
// against ALL observations of the track through the cameras' affine projections pix = A X + b; the inlier mask of the
// best one is refined by refit_rounds rounds of (ray intersection over the mask, reprojection errors, new mask).
// tests/consensus_restatement.py is the definition in numpy; this file holds what the kernels, the C entries
// (consensus_api.hip) and the device-resident scene (scene_api.hip) share.
#pragma once
#include "ba_solve.h"

namespace osfm {

// Tracks of at most kConsensusShortLen observations get eight neighbouring lanes (lane = observation), longer ones
// a wave (lane = hypothesis); the workgroups of both kernels have 256 threads.
constexpr int kConsensusShortLen = 8;
constexpr int kConsensusShortTracks = 32;      // tracks per workgroup, short path
constexpr int kConsensusLongTracks = 4;        // tracks per workgroup, long path (a wave each)
constexpr int kConsensusMaxSample = 16;        // 120 hypotheses: two rounds of 64 lanes
constexpr int kConsensusChunk = 64;            // observations staged in LDS at a time (long path)

// per-camera table: rows of A [0..5], b [6..7], unit look direction [8..10]
constexpr int kConsensusCam = 12;

// the integer counters of osfm_consensus_stats, in its order
enum { kCsTested = 0, kCsClean, kCsRepaired, kCsUnsupported, kCsDegenerate, kCsUnsettled, kCsObsTested, kCsObsDropped,
       kCsHypotheses, kCsCounters };

// Outputs on the device; none may be null.  points_out: the consensus point of CLEAN / REPAIRED tracks, the input
// point of every other; err: the reprojection errors at points_out.
struct ConsensusOut {
    uint8_t *keep;                 // [O]
    int32_t *status;               // [M]
    double *points_out;            // [M][4]
    uint8_t *valid;                // [M]
    double *err;                   // [O]
    unsigned long long *counters;  // [kCsCounters], zeroed here
};

// what consensus_run writes, as work arrays of one call
struct ConsensusBuffers {
    DevArray keep, status, points, valid, err, counters;
    int alloc(int M, int O)
    {
        OSFM_RETURN_IF(keep.alloc((size_t)std::max(O, 1)));
        OSFM_RETURN_IF(status.alloc((size_t)std::max(M, 1) * 4));
        OSFM_RETURN_IF(points.alloc((size_t)std::max(M, 1) * 32));
        OSFM_RETURN_IF(valid.alloc((size_t)std::max(M, 1)));
        OSFM_RETURN_IF(err.alloc((size_t)std::max(O, 1) * 8));
        OSFM_RETURN_IF(counters.alloc(sizeof(unsigned long long) * kCsCounters));
        return OSFM_OK;
    }
    ConsensusOut out() const
    {
        return ConsensusOut{ keep.as<uint8_t>(), status.as<int32_t>(), points.as<double>(), valid.as<uint8_t>(), err.as<double>(),
            counters.as<unsigned long long>() };
    }
};

// options checked by the caller (consensus_check_options).  d: a finished DeviceProblem's BaDev (cams / points as they
// are, lm == nullptr).  Work arrays come from the pool; nothing is synchronised.
int consensus_check_options(const osfm_consensus_options *o, const char *what);
int consensus_run(const BaDev &d, const osfm_consensus_options &o, const ConsensusOut &out, hipStream_t s);
void consensus_fill_stats(const unsigned long long *counters, float device_ms, osfm_consensus_stats *stats);

}  // namespace osfm
