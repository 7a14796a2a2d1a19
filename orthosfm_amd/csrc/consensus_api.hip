// C entries of the per-track consensus triangulation on a caller's problem (include/osfm_hip.h; the scene's entry is
// in scene_api.hip).  The estimator is consensus_kernels.hip's.
#include <vector>

#include "consensus_kernels.h"

using namespace osfm;

extern "C" {

void osfm_consensus_options_default(osfm_consensus_options *o)
{
    if (!o) return;
    o->max_error = 1.5;
    o->min_support = 3;
    o->max_sample = kConsensusMaxSample;
    o->refit_rounds = 2;
    o->device = 0;
}

void osfm_consensus_get_limits(osfm_consensus_limits *l)
{
    if (!l) return;
    l->short_length = kConsensusShortLen;
    l->short_tracks = kConsensusShortTracks;
    l->long_tracks = kConsensusLongTracks;
    l->max_sample = kConsensusMaxSample;
}

int osfm_ba_consensus(const osfm_ba_problem *p, const osfm_consensus_options *opts, uint8_t *obs_keep, int32_t *track_status,
    double *points_out, uint8_t *point_valid, double *obs_err, osfm_consensus_stats *stats)
{
    osfm_consensus_options o;
    osfm_consensus_options_default(&o);
    if (opts) o = *opts;
    OSFM_RETURN_IF(consensus_check_options(&o, "ba_consensus"));
    Layout L;                 // declared before the stream lease: it must outlive the copies that read it
    OSFM_RETURN_IF(validate_ba_problem(p, "ba_consensus", &L));
    OSFM_RETURN_IF(select_device(o.device));
    StreamLease sg;
    OSFM_RETURN_IF(sg.acquire());
    DeviceProblem D;
    OSFM_RETURN_IF(upload_ba_problem(p, L, 1.0, 3, sg.s, &D));
    const int M = p->num_points, O = p->num_observations;
    ConsensusBuffers B;
    OSFM_RETURN_IF(B.alloc(M, O));
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].a, sg.s));
    OSFM_RETURN_IF(consensus_run(D.dev, o, B.out(), sg.s));
    OSFM_HIP_CHECK(hipEventRecord(sg.ev[0].b, sg.s));
    unsigned long long counters[kCsCounters];
    OSFM_HIP_CHECK(hipMemcpyAsync(counters, B.counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, sg.s));
    if (obs_keep && O) OSFM_HIP_CHECK(hipMemcpyAsync(obs_keep, B.keep.ptr, (size_t)O, hipMemcpyDeviceToHost, sg.s));
    if (track_status && M) OSFM_HIP_CHECK(hipMemcpyAsync(track_status, B.status.ptr, (size_t)M * 4, hipMemcpyDeviceToHost, sg.s));
    if (points_out && M) OSFM_HIP_CHECK(hipMemcpyAsync(points_out, B.points.ptr, (size_t)M * 32, hipMemcpyDeviceToHost, sg.s));
    if (point_valid && M) OSFM_HIP_CHECK(hipMemcpyAsync(point_valid, B.valid.ptr, (size_t)M, hipMemcpyDeviceToHost, sg.s));
    if (obs_err && O) OSFM_HIP_CHECK(hipMemcpyAsync(obs_err, B.err.ptr, (size_t)O * 8, hipMemcpyDeviceToHost, sg.s));
    OSFM_HIP_CHECK(hipStreamSynchronize(sg.s));
    if (stats) {
        float ms = 0.0f;
        OSFM_HIP_CHECK(hipEventElapsedTime(&ms, sg.ev[0].a, sg.ev[0].b));
        consensus_fill_stats(counters, ms, stats);
    }
    return OSFM_OK;
}

}  // extern "C"
