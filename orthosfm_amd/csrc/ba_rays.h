// The rays of the orthographic cameras and the symmetric 3 x 3 eigensolver of the ray intersection, as device code
// shared by the kernels that triangulate: ba_triangulate_kernel (ba_kernels.hip) and the masked refit of the
// consensus filter (consensus_kernels.hip).  One operation order throughout (files that include this are built
// without FMA contraction).
//   triangulateOrthographicTracks + intersectRays: src/triangulation/triangulation.cpp:11-93; camera accessors
//   OrthoQuaternionCamera.cpp:45-59, OrthographicCamera.cpp:63-95,187-193
#pragma once
#include "ba_device.h"

namespace osfm {

__device__ __forceinline__ void quat_rot(const double *q, const double v[3], double out[3])
{
    const double u[3] = { q[0], q[1], q[2] };
    double t[3];
    cross3(u, v, t);
    t[0] *= 2.0; t[1] *= 2.0; t[2] *= 2.0;
    double ut[3];
    cross3(u, t, ut);
    out[0] = v[0] + q[3] * t[0] + ut[0];
    out[1] = v[1] + q[3] * t[1] + ut[1];
    out[2] = v[2] + q[3] * t[2] + ut[2];
}

__device__ inline void camera_ray(const BaDev &d, int c, double x, double y, double origin[3], double dir[3])
{
    const double *cam = d.cams + 7 * c;
    const double W = (double)d.img_w[c], H = (double)d.img_h[c];
    if (d.model == kModelQuat) {
        const double xn = -2.0 * ((x / W) - 0.5) + cam[4];
        const double yn = -2.0 * ((y / H) - 0.5) + cam[5];
        const double loc[3] = { cam[6] * xn, cam[6] * yn, -10.0 };
        const double z[3] = { 0.0, 0.0, 1.0 };
        quat_rot(cam, loc, origin);
        quat_rot(cam, z, dir);
    } else {
        const double om = cam[1] + 0.5 * 3.14159265358979323846, ph = cam[0], ro = cam[2];
        const double Ry[3][3] = { { cos(ro), -sin(ro), 0 }, { sin(ro), cos(ro), 0 }, { 0, 0, 1 } };
        const double Rx[3][3] = { { 1, 0, 0 }, { 0, cos(om), -sin(om) }, { 0, sin(om), cos(om) } };
        const double Rz[3][3] = { { cos(ph), -sin(ph), 0 }, { sin(ph), cos(ph), 0 }, { 0, 0, 1 } };
        double A[3][3], S[3][3];
        mat3_mul(Rz, Rx, A);
        mat3_mul(A, Ry, S);
        const double xn = -2.0 * ((x / W) - 0.5) + cam[3];
        const double yn = -2.0 * ((y / H) - 0.5) + cam[4];
        // toCameraSpace(v) = T^T S v = (s0, s2, -s1)
        auto tcs = [&](double v0, double v1, double v2, double o[3]) {
            const double s0 = S[0][0] * v0 + S[0][1] * v1 + S[0][2] * v2;
            const double s1 = S[1][0] * v0 + S[1][1] * v1 + S[1][2] * v2;
            const double s2 = S[2][0] * v0 + S[2][1] * v1 + S[2][2] * v2;
            o[0] = s0; o[1] = s2; o[2] = -s1;
        };
        double ax[3], ay[3], org[3];
        tcs(1, 0, 0, ax);
        tcs(0, 1, 0, ay);
        tcs(0, 0, -10.0, org);
        tcs(0, 0, 1, dir);
        for (int i = 0; i < 3; ++i) origin[i] = org[i] + xn * ax[i] * cam[5] + yn * ay[i] * cam[5];
    }
}

__device__ inline void eig3_jacobi(double A[3][3], double V[3][3], double w[3])
{
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off < 1e-300) break;
        for (int pp = 0; pp < 2; ++pp)
            for (int q = pp + 1; q < 3; ++q) {
                if (fabs(A[pp][q]) < 1e-300) continue;
                const double th = (A[q][q] - A[pp][pp]) / (2.0 * A[pp][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; ++k) {
                    const double akp = A[k][pp], akq = A[k][q];
                    A[k][pp] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    const double apk = A[pp][k], aqk = A[q][k];
                    A[pp][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][pp], vkq = V[k][q];
                    V[k][pp] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// Eigen's default rank cut of bdcSvd().solve on the eigenvalues w of R = sum (I - d d^T): x = sum v (v^T q) / lambda
// over the eigenvalues above 3 * 2^-52 * lambda_max
__device__ inline void solve_ray_system(double R[3][3], const double q[3], double x[3])
{
    double A[3][3], V[3][3], w[3];
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) A[a][b] = R[a][b];
    eig3_jacobi(A, V, w);
    const double wmax = fmax(fabs(w[0]), fmax(fabs(w[1]), fabs(w[2])));
    const double thr = fmax(wmax * 3.0 * 2.220446049250313e-16, 2.2250738585072014e-308);
    x[0] = 0.0; x[1] = 0.0; x[2] = 0.0;
    for (int i = 0; i < 3; ++i) {
        if (!(fabs(w[i]) > thr)) continue;
        const double c = (V[0][i] * q[0] + V[1][i] * q[1] + V[2][i] * q[2]) / w[i];
        x[0] += c * V[0][i]; x[1] += c * V[1][i]; x[2] += c * V[2][i];
    }
}

}  // namespace osfm
