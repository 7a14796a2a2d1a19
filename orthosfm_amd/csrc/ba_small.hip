// The one-workgroup form of the bundle adjustment: a problem of at most kSmallMaxCams cameras --
// the three-camera local adjustments of the incremental reconstruction -- start to finish in ONE launch of ONE
// workgroup: Jacobi scaling, first linearisation, every Levenberg-Marquardt iteration and the accept / reject control
// that ba_lm_decide / ba_lm_post take in the general form (ba_solve.hip: four launches and a host read per iteration,
// each kernel too short to fill the device).
//
// The arithmetic is the general form's, through ba_device.h and lm_*_logic of ba_kernels.h; only the order of the
// sums that cross threads differs.  Every such sum has a fixed order (a thread walks its tracks chunk after chunk;
// then the lanes of a wave in a fixed order, then the four waves) and there are no atomics: the solve repeats to the bit.
//
//   LDS      the camera tables of both iterates, the cameras' layout, Jacobi scales and LM diagonal, the reduced
//            camera system (<= 48 unknowns), its factor (in place), the right-hand side, the step, the reductions
//   memory   points, per-observation records, per-point V^-1 / gradient / diagonal (L2-resident at these sizes)
//
// Safety: every loop is bounded (max_num_iterations, M, O, the system size), every branch around a barrier is on a
// value all threads read from LDS behind a barrier, and nothing waits for another workgroup.
#include "ba_kernels.h"

namespace osfm {

namespace {

constexpr int kThreads = 256;
constexpr int kNc = kSmallMaxCams * 6;       // unknowns of the reduced camera system at most
constexpr int kLd = kNc + 1;                 // (odd: the lanes' column reads fall on different banks)

struct SmallLds {
    double S[kNc][kLd];                      // lower triangle; the Cholesky factor in place
    double rhs[kNc], y[kNc], diag_c[kNc], scale_c[kNc];
    double tab[2][kSmallMaxCams * kCamDer];  // camera tables (ba_device.h) of the two iterate buffers
    double part_cam[2 * kSmallMaxCams], gmax_cam[kSmallMaxCams];
    double xch[4][kPairSums][65];            // a pair's 54 sums of every lane on their way to their owners (65: banks)
    double tot[kPairSums];
    double red[4][4];
    double bcast;
    int32_t cam_ldim[kSmallMaxCams], cam_off[kSmallMaxCams];
    int32_t info;
    LmDev lm;
};

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ double wave_total(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ double wave_largest(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// the workgroup's totals (maxima where max_mask has the bit) of four values at once, the same in every thread: butterfly
// in the wave, then waves 0..3.  All threads call.
__device__ __forceinline__ void block_all4(double (&v)[4], unsigned max_mask, double (*red)[4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (max_mask >> q) & 1 ? wave_largest(v[q]) : wave_total(v[q]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q)
        v[q] = (max_mask >> q) & 1 ? fmax(fmax(red[0][q], red[1][q]), fmax(red[2][q], red[3][q]))
                                   : ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

struct Pass { int mode, update_diag, want_gradient; double radius; };

// ---- point phase: a thread per track, kSmallTrackChunk tracks per round.  V_j, g_j in observation order (as the
// general form's window kernel sums them), the LM diagonal, V^-1, the records.  All threads call.
__device__ __forceinline__ void
point_phase(const BaDev &d, const SmallBaArgs &a, SmallLds &L, const double *tab, const Pass &ps, double &cost, double &gmax, double &bad)
{
    double c_sum = 0.0, g_max = 0.0;
    int not_pd = 0;
    for (int j0 = 0; j0 < d.M; j0 += kSmallTrackChunk) {
        const int j = j0 + (int)threadIdx.x;
        if (j >= d.M) continue;
        const int ks = d.pt_start[j], ke = d.pt_start[j + 1];
        PointDer pd;
        point_der(d, j, d.points + 4 * j, true, pd);
        double V[3][3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, g[3] = { 0, 0, 0 };
        for (int k = ks; k < ke; ++k) {
            const int c = d.obs_cam[k];
            ObsLin o;
            linearize_obs(d, k, c, L.cam_off[c] | (L.cam_ldim[c] << 24), tab, pd, o);
            c_sum += 0.5 * o.rho0;
            double w[kObsRec];
#pragma unroll
            for (int x = 0; x < 6; ++x) { w[kRecJc + x] = o.Jc[0][x]; w[kRecJc + 6 + x] = o.Jc[1][x]; w[kRecQ + x] = 0.0; }
#pragma unroll
            for (int x = 0; x < 3; ++x) { w[kRecJp + x] = o.Jp[0][x]; w[kRecJp + 3 + x] = o.Jp[1][x]; }
            w[kRecR] = o.r[0]; w[kRecR + 1] = o.r[1];
            double2 *dst = reinterpret_cast<double2 *>(a.obsrec + (size_t)k * kObsRec);
#pragma unroll
            for (int i = 0; i < kObsRec / 2; ++i) dst[i] = make_double2(w[2 * i], w[2 * i + 1]);
            if (d.pdim) {
#pragma unroll
                for (int x = 0; x < 3; ++x) {
                    g[x] += o.Jp[0][x] * o.r[0] + o.Jp[1][x] * o.r[1];
#pragma unroll
                    for (int y = 0; y <= x; ++y) V[x][y] += o.Jp[0][x] * o.Jp[0][y] + o.Jp[1][x] * o.Jp[1][y];
                }
            }
        }
        if (!d.pdim) continue;
        V[0][1] = V[1][0]; V[0][2] = V[2][0]; V[1][2] = V[2][1];
        if (ps.mode == kPassScaleInit) {
            // Jacobi scaling, once, from the unscaled column norms
            for (int x = 0; x < 3; ++x) a.scale_p[3 * j + x] = 1.0 / (1.0 + sqrt(V[x][x]));
            continue;
        }
        for (int x = 0; x < 3; ++x) {
            const double dp = ps.update_diag ? fmin(fmax(V[x][x], a.min_diag), a.max_diag) : a.diag_p[3 * j + x];
            if (ps.update_diag) a.diag_p[3 * j + x] = dp;
            V[x][x] += dp / ps.radius;
        }
        double Vi[3][3];
        bool ok = true;
        if (ke > ks) {
            ok = inv3_spd(V, Vi);
        } else {
            for (int x = 0; x < 3; ++x)
                for (int y = 0; y < 3; ++y) Vi[x][y] = x == y ? 1.0 / V[x][x] : 0.0;
        }
        if (!ok) not_pd = 1;
        for (int x = 0; x < 3; ++x) {
            a.ge[3 * j + x] = g[x];
            for (int y = 0; y < 3; ++y) a.vinv[9 * j + 3 * x + y] = ok ? Vi[x][y] : 0.0;
        }
        // Q = Jp V^-1 into the track's records (Jp back from the record this thread has just stored)
        for (int k = ks; k < ke; ++k) {
            double2 *rec2 = reinterpret_cast<double2 *>(a.obsrec + (size_t)k * kObsRec);
            double jp[6], qv[6];
#pragma unroll
            for (int i = 0; i < 3; ++i) { const double2 v = rec2[kRecJp / 2 + i]; jp[2 * i] = v.x; jp[2 * i + 1] = v.y; }
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    qv[3 * rr + t] = !ok ? 0.0 : jp[3 * rr] * Vi[0][t] + jp[3 * rr + 1] * Vi[1][t] + jp[3 * rr + 2] * Vi[2][t];
#pragma unroll
            for (int i = 0; i < 3; ++i) rec2[kRecQ / 2 + i] = make_double2(qv[2 * i], qv[2 * i + 1]);
        }
        if (ps.want_gradient && ke > ks) {
            // |Plus(x, -g) - x|_inf with the unscaled gradient
            double dl[3], out[4];
            for (int x = 0; x < 3; ++x) dl[x] = -g[x] / d.scale_p[3 * j + x];
            homog_plus(d.points + 4 * j, dl, out);
            for (int x = 0; x < 4; ++x) g_max = fmax(g_max, fabs(d.points[4 * j + x] - out[x]));
        }
    }
    double v[4] = { c_sum, g_max, (double)not_pd, 0.0 };
    block_all4(v, 0x6, L.red);
    cost = v[0]; gmax = v[1]; bad = v[2];
}

// ---- pair phase: camera pair after camera pair (c1 >= c2), each the work of the whole workgroup: a thread walks
// its tracks chunk after chunk with the pair's 54 sums in registers, the sums are reduced in a fixed order, and a
// fixed thread per entry finishes it into S / rhs / the LM diagonal in LDS.  Every block of the lower block triangle
// is written by every call (zeros where two cameras share no track).  All threads call; ends behind a barrier.
__device__ __forceinline__ void
pair_phase(const BaDev &d, const SmallBaArgs &a, SmallLds &L, const Pass &ps)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool with_b = d.pdim && ps.mode != kPassScaleInit;
    for (int c1 = 0; c1 < d.C; ++c1) {
        for (int c2 = ps.mode == kPassScaleInit ? c1 : 0; c2 <= c1; ++c2) {
            const int n1 = L.cam_ldim[c1], n2 = L.cam_ldim[c2], o1 = L.cam_off[c1], o2 = L.cam_off[c2];
            if (n1 == 0 || n2 == 0) continue;          // (uniform: no entry of S, no unknown)
            const bool diag_pair = c1 == c2;
            double s[kPairSums];     // 6x6 block, diagonal of Jc^T Jc, reduced rhs, gradient
#pragma unroll
            for (int v = 0; v < kPairSums; ++v) s[v] = 0.0;
            for (int j = tid; j < d.M; j += kSmallTrackChunk) {
                int ka = -1, kb = -1;
                for (int k = d.pt_start[j], ke = d.pt_start[j + 1]; k < ke; ++k) {
                    const int c = d.obs_cam[k];
                    ka = c == c1 ? k : ka;
                    kb = c == c2 ? k : kb;
                }
                if (ka < 0 || kb < 0) continue;
                // of record a: Jc and Q; of record b: Jp and Jc (ba_kernels.h)
                double ra[kObsRec], rb[kRecQ];
                {
                    const double2 *pa = reinterpret_cast<const double2 *>(a.obsrec + (size_t)ka * kObsRec);
                    const double2 *pb = reinterpret_cast<const double2 *>(a.obsrec + (size_t)kb * kObsRec);
#pragma unroll
                    for (int i = kRecJc / 2; i < kObsRec / 2; ++i) { const double2 v = pa[i]; ra[2 * i] = v.x; ra[2 * i + 1] = v.y; }
#pragma unroll
                    for (int i = 0; i < kRecQ / 2; ++i) { const double2 v = pb[i]; rb[2 * i] = v.x; rb[2 * i + 1] = v.y; }
                }
                double Ja[2][6];
#pragma unroll
                for (int x = 0; x < 6; ++x) { Ja[0][x] = ra[kRecJc + x]; Ja[1][x] = ra[kRecJc + 6 + x]; }
                if (diag_pair) {
                    double rr0 = ra[kRecR], rr1 = ra[kRecR + 1];
#pragma unroll
                    for (int x = 0; x < 6; ++x) s[48 + x] += Ja[0][x] * rr0 + Ja[1][x] * rr1;
                    if (with_b) {
                        // rhs = Jc^T (r - Q g)
                        const double *gp = a.ge + 3 * j;
                        rr0 -= ra[kRecQ] * gp[0] + ra[kRecQ + 1] * gp[1] + ra[kRecQ + 2] * gp[2];
                        rr1 -= ra[kRecQ + 3] * gp[0] + ra[kRecQ + 4] * gp[1] + ra[kRecQ + 5] * gp[2];
                    }
#pragma unroll
                    for (int x = 0; x < 6; ++x) {
                        s[42 + x] += Ja[0][x] * rr0 + Ja[1][x] * rr1;
                        s[36 + x] += Ja[0][x] * Ja[0][x] + Ja[1][x] * Ja[1][x];
#pragma unroll
                        for (int y = 0; y < 6; ++y) s[6 * x + y] += Ja[0][x] * Ja[0][y] + Ja[1][x] * Ja[1][y];
                    }
                }
                if (with_b) {
                    // Z_a W_b^T = Jc_a^T (Q_a Jp_b^T) Jc_b
                    double Mq[2][2];
#pragma unroll
                    for (int r1 = 0; r1 < 2; ++r1)
#pragma unroll
                        for (int r2 = 0; r2 < 2; ++r2)
                            Mq[r1][r2] = ra[kRecQ + 3 * r1] * rb[kRecJp + 3 * r2] + ra[kRecQ + 3 * r1 + 1] * rb[kRecJp + 3 * r2 + 1] +
                                         ra[kRecQ + 3 * r1 + 2] * rb[kRecJp + 3 * r2 + 2];
#pragma unroll
                    for (int y = 0; y < 6; ++y) {
                        const double jb0 = rb[kRecJc + y], jb1 = rb[kRecJc + 6 + y];
                        const double t0 = Mq[0][0] * jb0 + Mq[0][1] * jb1;
                        const double t1 = Mq[1][0] * jb0 + Mq[1][1] * jb1;
#pragma unroll
                        for (int x = 0; x < 6; ++x) s[6 * x + y] -= Ja[0][x] * t0 + Ja[1][x] * t1;
                    }
                }
            }
            // fixed order: four neighbouring threads own a sum; each adds one wave's 64 lanes in lane order, then
            // (wave 0 + wave 1) + (wave 2 + wave 3).  (A butterfly per sum was 650 cross-lane operations per wave and pair.)
#pragma unroll
            for (int v = 0; v < kPairSums; ++v) L.xch[wave][v][lane] = s[v];
            __syncthreads();
            if (tid < 4 * kPairSums) {
                const int v = tid >> 2, w = tid & 3;
                double t = 0.0;
                for (int i = 0; i < 64; ++i) t += L.xch[w][v][i];
                t += __shfl_xor(t, 1);
                t += __shfl_xor(t, 2);
                if (w == 0) L.tot[v] = t;
            }
            __syncthreads();
            if (ps.mode == kPassScaleInit) {
                if (tid < n1) L.scale_c[o1 + tid] = 1.0 / (1.0 + sqrt(L.tot[36 + tid]));
            } else if (tid < 36) {
                const int x = tid / 6, y = tid - 6 * x;
                if (x < n1 && y < n2) {
                    double v = L.tot[tid];
                    if (diag_pair && x == y) {
                        const double dc = ps.update_diag ? fmin(fmax(L.tot[36 + x], a.min_diag), a.max_diag) : L.diag_c[o1 + x];
                        v += dc / ps.radius;
                    }
                    L.S[o1 + x][o2 + y] = v;
                }
            } else if (tid < 42) {
                const int x = tid - 36;
                if (diag_pair && x < n1 && ps.update_diag) L.diag_c[o1 + x] = fmin(fmax(L.tot[36 + x], a.min_diag), a.max_diag);
            } else if (tid < 48) {
                const int x = tid - 42;
                if (diag_pair && x < n1) L.rhs[o1 + x] = L.tot[tid];
            } else if (tid == 48 && diag_pair && ps.want_gradient) {
                // the camera's share of the gradient norm: |Plus(x, -g) - x|_inf, unscaled gradient
                double dl[6];
#pragma unroll
                for (int x = 0; x < 6; ++x) dl[x] = x < n1 ? -L.tot[48 + x] / L.scale_c[o1 + x] : 0.0;
                const double *cam = d.cams + 7 * c1;
                double out[7];
                for (int i = 0; i < 7; ++i) out[i] = cam[i];
                int t = 0;
                if (d.model == kModelQuat && d.cam_colmap[6 * c1] == 0) { quat_plus(cam, dl, out); t = 3; }
                for (; t < n1; ++t) {
                    const int f = d.cam_colmap[6 * c1 + t];
                    const int slot = d.model == kModelQuat ? f + 1 : f;
                    double dv = 0.0;
#pragma unroll
                    for (int x = 0; x < 6; ++x) dv = t == x ? dl[x] : dv;
                    out[slot] = cam[slot] + dv;
                }
                double gm = 0.0;
                for (int i = 0; i < 7; ++i) gm = fmax(gm, fabs(cam[i] - out[i]));
                L.gmax_cam[c1] = gm;
            }
            __syncthreads();
        }
    }
}

// ---- S y = rhs by wave 0, a lane per row (lane n: the right-hand side rides along as row n), rows in registers,
// column k through LDS; then x = L^-T y.  L.y: the solution (the camera step is -y); L.info: the first pivot that
// is not positive, + 1.  No barrier inside: one wave's LDS operations execute in order.  The caller's barrier follows.
__device__ __forceinline__ void
cholesky_wave(SmallLds &L, int n)
{
    const int i = threadIdx.x;
    if (i >= 64) return;                      // (no barrier in here)
    double row[kNc];
#pragma unroll
    for (int j = 0; j < kNc; ++j) row[j] = (j < n && i <= n && (j <= i || i == n)) ? (i < n ? L.S[i][j] : L.rhs[j]) : 0.0;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < kNc; ++k) {
        if (k < n) {                          // (no break: the rows stay in registers only while k is a constant)
            if (i == k) L.bcast = row[k];
            lds_fence();
            const double p = L.bcast;
            if (!(p > 0.0) && bad == 0) bad = k + 1;
            const double piv = sqrt(p);
            row[k] = i == k ? piv : row[k] / piv;
            if (i >= k && i < n) L.S[i][k] = row[k];
            lds_fence();
#pragma unroll
            for (int j = k + 1; j < kNc; ++j)
                if (j < n) row[j] -= row[k] * L.S[j][k];      // (entries right of the lane's diagonal are never read)
        }
    }
    // lane n holds y = L^-1 b
#pragma unroll
    for (int k = 0; k < kNc; ++k)
        if (i == n && k < n) L.y[k] = row[k];
    lds_fence();
    double acc = i < n ? L.y[i] : 0.0;
    lds_fence();
    for (int k = n - 1; k >= 0; --k) {
        if (i == k) L.y[k] = acc / L.S[k][k];
        lds_fence();
        if (i < k) acc -= L.S[k][i] * L.y[k];
    }
    if (i == 0) L.info = bad;
}

// ---- back phase: candidate points, the model cost change, the step norms and the candidate's cost; a thread per track
__device__ __forceinline__ void
back_phase(const BaDev &d, const SmallBaArgs &a, SmallLds &L, const double *cand_tab, double *points_out,
    double &mcc, double &sn, double &xn, double &ccost)
{
    double m_sum = 0.0, s_sum = 0.0, x_sum = 0.0, c_sum = 0.0;
    for (int j0 = 0; j0 < d.M; j0 += kSmallTrackChunk) {
        const int j = j0 + (int)threadIdx.x;
        if (j >= d.M) continue;
        const int ks = d.pt_start[j], ke = d.pt_start[j + 1];
        double step_p[3] = { 0, 0, 0 };
        if (d.pdim) {
            double t3[3] = { 0, 0, 0 };
            for (int k = ks; k < ke; ++k) {
                const double *rec = a.obsrec + (size_t)k * kObsRec;
                const int c = d.obs_cam[k], off = L.cam_off[c], n = L.cam_ldim[c];
                double u0 = 0.0, u1 = 0.0;
#pragma unroll
                for (int x = 0; x < 6; ++x)
                    if (x < n) { const double yx = L.y[off + x]; u0 += rec[kRecJc + x] * yx; u1 += rec[kRecJc + 6 + x] * yx; }
#pragma unroll
                for (int t = 0; t < 3; ++t) t3[t] += -(rec[kRecJp + t] * u0 + rec[kRecJp + 3 + t] * u1);
            }
            for (int t = 0; t < 3; ++t) t3[t] = a.ge[3 * j + t] + t3[t];
            const double *Vi = a.vinv + 9 * j;
            for (int x = 0; x < 3; ++x) step_p[x] = -(Vi[3 * x] * t3[0] + Vi[3 * x + 1] * t3[1] + Vi[3 * x + 2] * t3[2]);
        }
        const double *P = d.points + 4 * j;
        double out[4] = { P[0], P[1], P[2], P[3] };
        if (d.pdim) {
            double dl[3];
            for (int x = 0; x < 3; ++x) dl[x] = step_p[x] * d.scale_p[3 * j + x];
            homog_plus(P, dl, out);
            for (int x = 0; x < 4; ++x) { s_sum += (P[x] - out[x]) * (P[x] - out[x]); x_sum += P[x] * P[x]; }
        }
        for (int x = 0; x < 4; ++x) points_out[4 * j + x] = out[x];
        const double pc[3] = { out[0] / out[3], out[1] / out[3], out[2] / out[3] };
        for (int k = ks; k < ke; ++k) {
            const double *rec = a.obsrec + (size_t)k * kObsRec;
            const int c = d.obs_cam[k], off = L.cam_off[c], n = L.cam_ldim[c];
            double u0 = 0.0, u1 = 0.0;
#pragma unroll
            for (int x = 0; x < 6; ++x)
                if (x < n) { const double yx = L.y[off + x]; u0 += rec[kRecJc + x] * yx; u1 += rec[kRecJc + 6 + x] * yx; }
            // model_cost_change = -(J step)^T (r + J step / 2)
            double m0 = -u0, m1 = -u1;
#pragma unroll
            for (int t = 0; t < 3; ++t) { m0 += rec[kRecJp + t] * step_p[t]; m1 += rec[kRecJp + 3 + t] * step_p[t]; }
            m_sum += -(m0 * (rec[kRecR] + m0 / 2.0) + m1 * (rec[kRecR + 1] + m1 / 2.0));
            c_sum += 0.5 * obs_cost_at(d, k, cand_tab, kCamDer, pc);
        }
    }
    double v[4] = { m_sum, s_sum, x_sum, c_sum };
    block_all4(v, 0, L.red);
    mcc = v[0]; sn = v[1]; xn = v[2]; ccost = v[3];
}

__global__ __launch_bounds__(kThreads, 1) void
ba_small_kernel(BaDev d, SmallBaArgs a)
{
    __shared__ __attribute__((aligned(16))) SmallLds L;
    const int tid = threadIdx.x;
    const int n = d.nc;
    // ---- the tables: layout, scales of one, an empty system, the start cameras' rows, the state ----
    for (int i = tid; i < kNc * kLd; i += kThreads) (&L.S[0][0])[i] = 0.0;
    if (tid < kNc) { L.rhs[tid] = 0.0; L.y[tid] = 0.0; L.diag_c[tid] = 0.0; L.scale_c[tid] = 1.0; }
    if (tid < kSmallMaxCams) {
        L.cam_ldim[tid] = tid < d.C ? d.cam_ldim[tid] : 0;
        L.cam_off[tid] = tid < d.C ? d.cam_off[tid] : 0;
        L.gmax_cam[tid] = 0.0; L.part_cam[2 * tid] = 0.0; L.part_cam[2 * tid + 1] = 0.0;
    }
    if (tid == 0) {
        LmDev init = {};
        init.radius = a.radius0; init.decrease_factor = 2.0;
        init.update_diag = 1; init.want_gradient = 1; init.term = OSFM_BA_NO_CONVERGENCE;
        L.lm = init;
        L.info = 0;
        a.stamps[0] = (long long)wall_clock64();
    }
    for (int i = tid; i < 3 * d.M; i += kThreads) a.scale_p[i] = 1.0;
    if (tid < 4 * d.C) {
        const int c = tid >> 2;
        cam_derive_part(d.model, d.cams2[0] + 7 * c, (double)d.img_w[c], (double)d.img_h[c], d.cam_colmap + 6 * c, d.cam_ldim[c],
            tid & 3, true, &L.tab[0][kCamDer * c]);
    }
    d.scale_c = L.scale_c; d.scale_p = a.scale_p;
    d.cams = d.cams2[0]; d.points = d.points2[0];
    __syncthreads();

    Pass ps;
    double cost, gp, bad;
    if (a.jacobi_scaling) {
        ps.mode = kPassScaleInit; ps.update_diag = 0; ps.want_gradient = 0; ps.radius = a.radius0;
        point_phase(d, a, L, L.tab[0], ps, cost, gp, bad);
        __syncthreads();
        pair_phase(d, a, L, ps);
    }
    // a linearisation at the current iterate and the control behind it (ba_lm_post); all threads, ends behind a barrier
    auto linearize = [&](int initial) {
        const int cur = L.lm.cur;
        ps.mode = kPassNormal; ps.update_diag = L.lm.update_diag; ps.want_gradient = L.lm.want_gradient; ps.radius = L.lm.radius;
        d.cams = cur ? d.cams2[1] : d.cams2[0];
        d.points = cur ? d.points2[1] : d.points2[0];
        point_phase(d, a, L, cur ? L.tab[1] : L.tab[0], ps, cost, gp, bad);
        __syncthreads();
        pair_phase(d, a, L, ps);
        if (tid == 0) {
            double gc = 0.0;
            for (int c = 0; c < d.C; ++c) gc = fmax(gc, L.gmax_cam[c]);
            lm_post_logic(&L.lm, a.prm, initial, cost, gp, bad, gc);
        }
        __syncthreads();
    };
    linearize(1);
    if (tid == 0) a.stamps[1] = (long long)wall_clock64();

    LmScratch sc = {};
    sc.chol_info = &L.info;
    for (int it = 0; it <= a.prm.max_iterations; ++it) {
        if (L.lm.stop) break;                 // (the same in every thread: read behind a barrier, written behind the next)
        const bool solved = !L.lm.lin_failed;
        const int cur = L.lm.cur;
        double mcc = 0.0, sn = 0.0, xn = 0.0, ccost = 0.0;
        __syncthreads();
        if (solved) {
            cholesky_wave(L, n);
            __syncthreads();
            // the candidate cameras, four lanes each: the candidate, its norms, a quarter of its table row
            double *cams_out = cur ? d.cams2[0] : d.cams2[1];
            double *tab_out = cur ? L.tab[0] : L.tab[1];
            if (tid < 4 * d.C) {
                const int c = tid >> 2, part = tid & 3;
                double out[7], csn, cxn;
                cam_candidate(d, L.y, c, out, csn, cxn);
                if (part == 0) {
                    for (int i = 0; i < 7; ++i) cams_out[7 * c + i] = out[i];
                    L.part_cam[2 * c] = csn; L.part_cam[2 * c + 1] = cxn;
                }
                cam_derive_part(d.model, out, (double)d.img_w[c], (double)d.img_h[c], d.cam_colmap + 6 * c, d.cam_ldim[c], part, true,
                    tab_out + kCamDer * c);
            }
            __syncthreads();
            back_phase(d, a, L, tab_out, cur ? d.points2[0] : d.points2[1], mcc, sn, xn, ccost);
        }
        if (tid == 0) {
            for (int c = 0; c < d.C; ++c) { sn += L.part_cam[2 * c]; xn += L.part_cam[2 * c + 1]; }
            lm_decide_logic(&L.lm, a.prm, sc, solved, mcc, sn, xn, ccost);
        }
        __syncthreads();
        if (!L.lm.stop) linearize(0);
    }
    __syncthreads();
    if (tid == 0) {
        *a.lm = L.lm;
        a.stamps[2] = (long long)wall_clock64();
    }
}

}  // namespace

void launch_small_ba(const BaDev &d, const SmallBaArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(ba_small_kernel, dim3(1), dim3(kThreads), 0, s, d, a);
}

}  // namespace osfm
