// The depth refinement's arithmetic as plain inline C++: the kernels of icp_kernels.h call it on the device,
// tests/native/icp_host.cpp calls the same text from serial loops on the host.
//
// What it restates (paths relative to the reference's auto_pose/):
//   points      ae/pysixd_stuff/misc.py:65-76 (rgbd_to_point_cloud: nonzero pixels in row-major order, float64 from the fp32 depth)
//   filter      eval/icp_utils.py:251-261, icp/icp.py:164-174 (centroid, largest distance, real points inside factor * that)
//   one step    eval/icp_utils.py:139-163 (nearest target, best_fit_transform, src = T src, the stop test)
//   solve       eval/icp_utils.py:21-74, icp/icp.py:18-69 (centroids, H = AA^T BB, SVD, R = V U^T, reflection, the translation rules)
//
// The exactness rule.  Everything is float64 in one fixed order of operations with contraction off, so the host driver and
// the kernels agree bit for bit: the nearest neighbour is the smallest (d^2, index) key -- independent of how the scan is
// split -- and every sum is "accumulators in a fixed lane pattern, then a fixed tree" (icp_tree_*), or 64-point block
// partials added in block order.  Against the reference (NumPy sums in another order, LAPACK's SVD) the transforms agree to
// rounding, not bitwise.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ICP_HD __host__ __device__ inline
#else
#define ICP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace aae_icp {

#define ICP_MAX_PROBLEMS 16                       /* problems per call (the table travels in the kernel arguments)          */
#define ICP_MAX_POINTS 4096                       /* subsampled points per problem: 4096 x 24 B of targets = 96 KB of LDS    */
#define ICP_BLOCK_POINTS 64                       /* source points of one icp_step block = one partial                      */
#define ICP_MAX_BLOCKS (ICP_MAX_POINTS / ICP_BLOCK_POINTS)
#define ICP_LANES 256                             /* accumulator lanes of a fixed-order sum (icp_stats, icp_finish)         */
#define ICP_NQ 16                                 /* sums of one partial: src[3], dst[3], src dst^T [9], distance           */
#define ICP_SVD_SWEEPS 30                         /* bound of the Jacobi sweeps (3x3: converged after 4-6)                  */

#define ICP_DEPTH_ONLY 1                          /* R = I, t = (0, 0, dz)                                                   */
#define ICP_NO_DEPTH 2                            /* the translation's z is dropped ...                                      */
#define ICP_NO_DEPTH_ZERO_T 4                     /* ... or all of it (icp/icp.py:58-61)                                     */

#define ICP_ERR_INDEX 1                           /* error word: a subsample index outside [0, count) was clamped            */

struct IcpCamera {
    double K00, K02, K11, K12;                    // the entries rgbd_to_point_cloud reads
};

// ---- points ----------------------------------------------------------------------------------------------------------
// misc.py:66 keeps depth != 0 (a negative or NaN pixel is a point too)
ICP_HD bool icp_is_point(float depth) { return depth != 0.0f; }

// misc.py:67-70: xs = ((us - K02) * zs) / K00, ys = ((vs - K12) * zs) / K11, in float64 from the float32 depth
ICP_HD void icp_backproject(const IcpCamera& cam, int u, int v, float depth, double* p) {
    const double z = (double)depth;
    p[0] = (((double)u - cam.K02) * z) / cam.K00;
    p[1] = (((double)v - cam.K12) * z) / cam.K11;
    p[2] = z;
}

ICP_HD double icp_dist2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// icp_utils.py:260-261: norm(p - centroid) < factor * max_mean_dist (thresh is that product, formed once)
ICP_HD bool icp_filter_keeps(const double* p, const double* centroid, double thresh) {
    return sqrt(icp_dist2(p[0], p[1], p[2], centroid[0], centroid[1], centroid[2])) < thresh;
}

// ---- the arg-min key: smaller d^2, then lower index --------------------------------------------------------------------
ICP_HD bool icp_key_less(double d2a, int ia, double d2b, int ib) { return d2a < d2b || (d2a == d2b && ia < ib); }

// ---- fixed-order sums -------------------------------------------------------------------------------------------------
// value i of a list goes to accumulator lane i % ICP_LANES, in ascending i; then a[k] += a[k + s] for s = 128, 64 ... 1.
// (the host runs the lanes one after the other, the device one thread per lane: the same additions)
ICP_HD void icp_tree_sum(double* a) {
    for (int s = ICP_LANES / 2; s > 0; s >>= 1)
        for (int k = 0; k < s; ++k) a[k] += a[k + s];
}

// one correspondence's contribution to the 16 sums, about the problem's origin o (nothing large is ever subtracted)
ICP_HD void icp_pair_terms(const double* src, const double* dst, const double* o, double dist, double* q) {
    const double a0 = src[0] - o[0], a1 = src[1] - o[1], a2 = src[2] - o[2];
    const double b0 = dst[0] - o[0], b1 = dst[1] - o[1], b2 = dst[2] - o[2];
    q[0] = a0; q[1] = a1; q[2] = a2;
    q[3] = b0; q[4] = b1; q[5] = b2;
    q[6] = a0 * b0; q[7] = a0 * b1; q[8] = a0 * b2;
    q[9] = a1 * b0; q[10] = a1 * b1; q[11] = a1 * b2;
    q[12] = a2 * b0; q[13] = a2 * b1; q[14] = a2 * b2;
    q[15] = dist;
}

// ---- the 3x3 rotation: R = V U^T of H = U S V^T, the reflection fix on the smallest singular value -------------------------
ICP_HD double icp_det3(const double* m) {
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// One-sided Jacobi: G = H V with orthogonal columns, V a product of plane rotations; singular values are the column
// norms.  U's columns: the largest two from G (re-orthogonalised), the third their cross product signed like G's third
// column -- exact also where the smallest singular value is 0 (rank 2) and its column of G is noise.
template <int P, int Q>
ICP_HD bool icp_jacobi_pair(double* G, double* V) {
    const double alpha = (G[P] * G[P] + G[3 + P] * G[3 + P]) + G[6 + P] * G[6 + P];
    const double beta = (G[Q] * G[Q] + G[3 + Q] * G[3 + Q]) + G[6 + Q] * G[6 + Q];
    const double gamma = (G[P] * G[Q] + G[3 + P] * G[3 + Q]) + G[6 + P] * G[6 + Q];
    if (!(fabs(gamma) > 1e-16 * sqrt(alpha * beta))) return false;                  // (also skips NaN)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    for (int r = 0; r < 3; ++r) {
        const double gp = G[3 * r + P], gq = G[3 * r + Q];
        G[3 * r + P] = c * gp - s * gq;
        G[3 * r + Q] = s * gp + c * gq;
        const double vp = V[3 * r + P], vq = V[3 * r + Q];
        V[3 * r + P] = c * vp - s * vq;
        V[3 * r + Q] = s * vp + c * vq;
    }
    return true;
}

template <int I, int J>
ICP_HD void icp_order_cols(double* G, double* V, double* sv) {                       // the larger singular value in front
    if (!(sv[J] > sv[I])) return;
    double t = sv[I]; sv[I] = sv[J]; sv[J] = t;
    for (int r = 0; r < 3; ++r) {
        t = G[3 * r + I]; G[3 * r + I] = G[3 * r + J]; G[3 * r + J] = t;
        t = V[3 * r + I]; V[3 * r + I] = V[3 * r + J]; V[3 * r + J] = t;
    }
}

ICP_HD void icp_rotation_from_H(const double* H, double* R) {
    double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) G[i] = H[i];
    for (int sweep = 0; sweep < ICP_SVD_SWEEPS; ++sweep) {
        const bool r01 = icp_jacobi_pair<0, 1>(G, V), r02 = icp_jacobi_pair<0, 2>(G, V), r12 = icp_jacobi_pair<1, 2>(G, V);
        if (!(r01 || r02 || r12)) break;
    }
    double sv[3];
    for (int k = 0; k < 3; ++k) sv[k] = sqrt((G[k] * G[k] + G[3 + k] * G[3 + k]) + G[6 + k] * G[6 + k]);
    icp_order_cols<0, 1>(G, V, sv);                                                  // descending, stable
    icp_order_cols<1, 2>(G, V, sv);
    icp_order_cols<0, 1>(G, V, sv);
    double u0[3] = {1, 0, 0}, u1[3], u2[3];
    if (sv[0] > 0.0)
        for (int r = 0; r < 3; ++r) u0[r] = G[3 * r] / sv[0];
    // second column: G's, made orthogonal to the first; without one (rank <= 1) the axis least aligned with u0
    const double d = (u0[0] * G[1] + u0[1] * G[4]) + u0[2] * G[7];
    for (int r = 0; r < 3; ++r) u1[r] = G[3 * r + 1] - d * u0[r];
    double n1 = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    if (!(n1 > 1e-14 * sv[0]) || !(n1 > 0.0)) {
        const bool ax0 = fabs(u0[0]) <= fabs(u0[1]) && fabs(u0[0]) <= fabs(u0[2]);
        const bool ax1 = !ax0 && fabs(u0[1]) <= fabs(u0[2]);
        const double e[3] = {ax0 ? 1.0 : 0.0, ax1 ? 1.0 : 0.0, (!ax0 && !ax1) ? 1.0 : 0.0};
        const double ua = (e[0] * u0[0] + e[1] * u0[1]) + e[2] * u0[2];
        for (int r = 0; r < 3; ++r) u1[r] = e[r] - ua * u0[r];
        n1 = sqrt((u1[0] * u1[0] + u1[1] * u1[1]) + u1[2] * u1[2]);
    }
    for (int r = 0; r < 3; ++r) u1[r] /= n1;
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    if ((u2[0] * G[2] + u2[1] * G[5]) + u2[2] * G[8] < 0.0)
        for (int r = 0; r < 3; ++r) u2[r] = -u2[r];
    // R = V U^T (icp_utils.py:53); det R < 0: the last row of Vt -- the smallest singular value's -- changes sign (:55-57)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (V[3 * i] * u0[j] + V[3 * i + 1] * u1[j]) + V[3 * i + 2] * u2[j];
    if (icp_det3(R) < 0.0)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = (V[3 * i] * u0[j] + V[3 * i + 1] * u1[j]) - V[3 * i + 2] * u2[j];
}

// ---- best_fit_transform from the 16 sums of n correspondences about the origin o -----------------------------------------
// T: 4x4 row major.  Returns the sum of distances / n (np.mean(distances)).
ICP_HD double icp_solve(const double* S, int n, const double* o, int mode, double* T) {
    const double dn = (double)n;
    const double ma[3] = {S[0] / dn, S[1] / dn, S[2] / dn}, mb[3] = {S[3] / dn, S[4] / dn, S[5] / dn};
    const double ca[3] = {o[0] + ma[0], o[1] + ma[1], o[2] + ma[2]}, cb[3] = {o[0] + mb[0], o[1] + mb[1], o[2] + mb[2]};
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3];
    if (mode & ICP_DEPTH_ONLY) {
        t[0] = 0.0; t[1] = 0.0; t[2] = mb[2] - ma[2];                              // icp_utils.py:45-48
    } else {
        double H[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[3 * r + c] = S[6 + 3 * r + c] - S[r] * mb[c];      // sum (a - ma)(b - mb)^T
        icp_rotation_from_H(H, R);
        for (int r = 0; r < 3; ++r) t[r] = cb[r] - ((R[3 * r] * ca[0] + R[3 * r + 1] * ca[1]) + R[3 * r + 2] * ca[2]);
        if (mode & ICP_NO_DEPTH) {
            t[2] = 0.0;                                                            // icp_utils.py:60-61
            if (mode & ICP_NO_DEPTH_ZERO_T) t[0] = t[1] = 0.0;                     // icp/icp.py:58-61
        }
    }
    for (int r = 0; r < 3; ++r) {
        T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2]; T[4 * r + 3] = t[r];
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    return S[15] / dn;
}

// src = T src (icp_utils.py:155)
ICP_HD void icp_apply(const double* T, double* p) {
    const double x = p[0], y = p[1], z = p[2];
    p[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    p[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    p[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// icp_utils.py:158-163 after one more iteration: the state of a problem between two steps
struct IcpState {
    double prev_error;                            // starts at 0, updated only when the loop goes on
    double mean_error;                            // of the last iteration that ran
    int32_t iterations;                           // iterations that ran; the reference's i is this - 1
    int32_t done;
};

ICP_HD void icp_advance(IcpState* s, double mean_error, double tolerance, int max_iterations) {
    s->mean_error = mean_error;
    s->iterations += 1;
    if (fabs(s->prev_error - mean_error) < tolerance) s->done = 1;
    else s->prev_error = mean_error;
    if (s->iterations >= max_iterations) s->done = 1;
}

}  // namespace aae_icp
