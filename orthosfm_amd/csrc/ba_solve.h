// The bundle-adjustment solve on device-resident arrays: what osfm_ba_solve (host arrays in, host arrays out)
// and the device-resident scene (scene_api.hip: the arrays never leave the device) both run.  The problem is built
// by ba_api.hip / scene_api.hip, solved by ba_solve.hip.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "ba_kernels.h"
#include "osfm_common.h"

namespace osfm {

// a work array of one call, from the pool of osfm_common.h
struct DevArray {
    void *ptr = nullptr;
    DevArray() = default;
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
    ~DevArray() { if (ptr) pool_release(ptr); }
    int alloc(size_t bytes)
    {
        if (ptr) { pool_release(ptr); ptr = nullptr; }
        return g_device_pool.alloc(&ptr, std::max<size_t>(bytes, 16));
    }
    template <typename T> T *as() const { return static_cast<T *>(ptr); }
};

template <typename T>
int upload(DevArray &d, const T *src, size_t n, hipStream_t s)
{
    OSFM_RETURN_IF(d.alloc(n * sizeof(T)));
    if (n) OSFM_HIP_CHECK(hipMemcpyAsync(d.ptr, src, n * sizeof(T), hipMemcpyHostToDevice, s));
    return OSFM_OK;
}

// tangent layout of the camera blocks (host side; pt_start only where the observations are the caller's)
struct Layout {
    std::vector<int32_t> cam_ldim, cam_off, pt_start;
    std::vector<int8_t> colmap;
    int nc = 0;
};

// An elimination order of the reduced camera system for banded (ring / strip) visibility: ba_order.hip
struct ReducedOrder {
    bool active = false;
    int span = 0;                             // unknowns of the laid-out system, interior padding included
    int nblk = 0;                             // blocks of 32 of it
    int arcs = 0, sep_cams = 0;               // K arcs, separators of that many cameras
    int chain_natural = 0, chain_ordered = 0; // longest chain of dependent diagonal blocks, before / after
    std::vector<int32_t> cam_off;             // [C]
    std::vector<int32_t> pad;                 // padding unknowns below span (identity rows)
    std::vector<unsigned long long> nz;       // FlowPattern::nz
    std::vector<int32_t> ptiles;              // FlowPattern::ptiles
};
// pairs: the camera pairs (a >= b, a == b included or not) that share a track; ldim: unknowns per camera.  False
// (out->active == false, chain_natural filled in): the natural order stands.
bool choose_reduced_order(int C, const int32_t *ldim, const std::vector<std::pair<int, int>> &pairs, ReducedOrder *out);

// The problem as the triangulation, reprojection and LM kernels read it: the caller's arrays, the camera layout, and
// the second iterate buffers.  The solve only reads it; its scales, camera tables and LM state are its own.
struct DeviceProblem {
    DevArray cams[2], points[2], obs_xy, obs_cam, obs_pt, pt_start, img_w, img_h;
    DevArray cam_ldim, cam_off, colmap;
    BaDev dev;
};

// which columns of a camera block are free (SetupParameterBlocks, OrthoQuaternionRecoAlgorithm.cpp:121-148,
// OrthographicReconstructionAlgorithm.cpp:148-178), from the constancy masks [C][7]
void build_camera_layout(int model, int C, const uint8_t *cam_const, Layout *L);
// D->dev from the arrays D holds (cams[0], points[0], obs_*, pt_start, img_*, the camera layout); allocates the
// candidate buffers and the per-observation point index
int finish_device_problem(int model, int C, int M, int O, int nc, double huber, int pdim, hipStream_t s, DeviceProblem *D);

// osfm_ba_solve's checks of a caller's problem (sizes, model, null arrays, observation ranges and order, one observation
// per camera and point) with the caller's layout, and its upload into a finished DeviceProblem (L, which may have been
// rebuilt from other constancy masks, has to outlive the stream's next synchronisation)
int validate_ba_problem(const osfm_ba_problem *p, const char *what, Layout *L);
int upload_ba_problem(const osfm_ba_problem *p, const Layout &L, double huber, int pdim, hipStream_t s, DeviceProblem *D);

// The Levenberg-Marquardt solve (ba_solve.hip) on a finished DeviceProblem (start values in cams[0] / points[0]), which it
// leaves as it was.  pair_bound: an upper bound of the Schur pair entries (sum of squared track lengths), refused beyond
// 2^31 - 1.  On return *cur names the buffer pair (cams[cur], points[cur]) that holds the result; the stream is
// synchronised.  cap (test hook osfm_ba_debug_linearization; null in every solve): copies of the first iteration
// o.small_form (osfm_hip.h) picks between the general form and the one-workgroup form (ba_small.hip) here, so
// every caller honours it; both leave the same things behind.
int ba_solve_core(const DeviceProblem &D, const osfm_ba_options &o, StreamLease &sg, int64_t pair_bound, osfm_ba_summary *sum,
    int *cur, osfm_ba_lin_capture *cap = nullptr);
// osfm_ba_options::small_form against a problem of num_cameras cameras (capture: osfm_ba_debug_linearization):
// OSFM_E_ARG for a value that is none of 0, 1, 2 and for 2 where the one-workgroup form cannot run.  The entry
// points call it before they queue anything; ba_solve_core calls it too.
int check_small_form(const osfm_ba_options &o, int num_cameras, bool capture, const char *what);

// The dense Cholesky's buffers for a system of span unknowns, padded to N: S with the right-hand side in row N, the
// factor, Ldiag, the solution y; for the one-launch form (flow) its hand-off flags, zeroed here once, and mailbox
struct CholeskyBuffers {
    DevArray S, L, Ldiag, y, flags, mailbox;
    int N = 0, epoch = 0;             // epoch: differs from every earlier solve on the same flags
    size_t s_elems = 0;               // of S and L: (N + 32) x N
    bool flow = false;
    int alloc(int span, bool allow_flow, hipStream_t s)
    {
        const int n = std::max(span, 1);
        N = cholesky_padded_dim(n);
        s_elems = (size_t)(N + 32) * N;
        OSFM_RETURN_IF(S.alloc(s_elems * 8));
        OSFM_RETURN_IF(L.alloc(s_elems * 8));
        OSFM_RETURN_IF(Ldiag.alloc((size_t)N * 32 * 8));
        OSFM_RETURN_IF(y.alloc((size_t)N * 8));
        flow = allow_flow && N > 32;          // (a system of one block never takes the one-launch form: chol_small_kernel)
        if (flow) {
            OSFM_RETURN_IF(flags.alloc((size_t)chol_flow_flag_count(n) * 4));
            OSFM_HIP_CHECK(hipMemsetAsync(flags.ptr, 0, (size_t)chol_flow_flag_count(n) * 4, s));
            OSFM_RETURN_IF(mailbox.alloc(chol_flow_mailbox_bytes(n)));
        }
        return OSFM_OK;
    }
    // S (lower triangle) -> y; one_launch: the one-launch form where flow.  Returns 1 when that form ran
    int solve(int span, int *info, const LmDev *lm, bool one_launch, const FlowPattern &pattern, hipStream_t s, int max_d = 0, int max_groups = 0)
    {
        return launch_cholesky_solve(S.as<double>(), L.as<double>(), span, Ldiag.as<double>(), y.as<double>(), info, lm, s,
            one_launch ? flags.as<int>() : nullptr, ++epoch, one_launch ? mailbox.as<double>() : nullptr, pattern, max_d, max_groups);
    }
};

// where the caller's camera unknowns (ldim[c] per camera) sit in the laid-out system; cam_off (may be null): each camera's first
inline std::vector<int32_t> unknown_positions(int C, const int32_t *ldim, const ReducedOrder &ord, int32_t *cam_off = nullptr)
{
    std::vector<int32_t> pos;
    for (int c = 0, tot = 0; c < C; tot += ldim[c], ++c) {
        const int off = ord.active ? ord.cam_off[c] : tot;
        if (cam_off) cam_off[c] = off;
        for (int i = 0; i < ldim[c]; ++i) pos.push_back(off + i);
    }
    return pos;
}

// One linearisation of a finished DeviceProblem at its own cameras and points with the LM term OFF, by the solve's point
// and pair passes: radius = infinity makes every diagonal's share diag / radius an exact zero, so the kernels run as they
// are; unit Jacobi scales, the cameras' own order, launch-per-column Cholesky buffers.  What the passes left (all on
// the device, alive while the callbacks run):
struct PlainLin {
    const double *obsrec;         // [O][kObsRec] Jc, Jp, Q = Jp V_j^-1, r per observation (unscaled)
    const double *vinv;           // [9 M] V_j^-1
    const int32_t *obs_lay;       // [O] cam_off | cam_ldim << 24 of the observation's camera
    const double *cost_partials;  // [num_windows] the windows' shares of the cost, to be added in order
    int num_windows;
    CholeskyBuffers *chol;        // S (lower triangle blocks, identity on the padding diagonal) after the pair pass
    bool dense;                   // S's point part came from the dense product
};
// after_points runs behind the point pass (nonzero: returned as it is, nothing else happens), after_system behind the
// pair pass.  Neither stage synchronises.
int ba_linearize_plain(const DeviceProblem &D, StreamLease &sg, int64_t pair_bound,
    const std::function<int(const PlainLin &)> &after_points, const std::function<int(const PlainLin &)> &after_system);

using Clock = std::chrono::steady_clock;
inline void lap(int verbose, Clock::time_point t0, const char *what)       // verbose >= 2: the time since t0 on stderr
{
    if (verbose >= 2) fprintf(stderr, "[osfm ba] %-18s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(Clock::now() - t0).count());
}

int select_device(int device);

}  // namespace osfm
