// gsr_pose.hip -- relative-pose evaluation of the reference (src/evaluation/pose_evaluator.py) on the device:
//
// gsr_pnp_ransac: `get_pnp_pose` (src/misc/cam_utils.py:158-178) without the host round trip through cv2.solvePnPRansac, batched over P
//   independent problems (blockIdx.y).  The contract is the geometry, not OpenCV's random stream:
//   1. k_pnp_prefix   one block per problem: opacity mask counted per granule of 64 points, exclusive prefix over the granules.
//   2. k_pnp_hypo     one thread per hypothesis, float64: six masked points drawn with a counter-based generator keyed by
//                     (seed, hypothesis, draw) -- the r-th masked point is found through the prefix, so no state and no dependence
//                     on the launch shape; the problem's index is NOT part of the key, or its result would depend on its place in
//                     a batch -- then a 6-point DLT on centred / scaled points (11 of the 12 equations, p34 = 1:
//                     after centring p34 is the depth of the sample's centroid), the rotation by Newton's polar iteration, and
//                     Gauss-Newton on the six reprojection errors.  Repeated points, a vanishing pivot, det <= 0 or a sample point
//                     behind the camera make the hypothesis invalid.
//   3. k_pnp_score    every hypothesis against every masked point in fp32: 1024 points per block held in registers, the poses of 128
//                     hypotheses at a time in LDS (wave-uniform reads), inliers counted by ballot, integer adds.
//   4. k_pnp_select   largest count, ties to the lowest index.
//   5. k_pnp_accum + k_pnp_step, PNP_REFINE times: Levenberg-Marquardt on the left-multiplicative 6-DoF update T <- SE3_exp(d) T.
//                     k_pnp_accum evaluates the candidate pose: per-block float64 partial sums of the 21 + 6 normal-equation terms over
//                     the points within the reprojection bound and of the truncated cost sum(min(r^2, bound^2)) over all masked
//                     points; k_pnp_step folds them in block order, accepts the candidate iff the truncated cost fell, and solves the
//                     damped 6 x 6 system in one thread.  The inlier set is therefore re-evaluated under every accepted pose.
//   6. k_pnp_finish   inlier mask and count under the final pose in float64, c2w = (R|t)^-1.
//   Failure (fewer than 6 masked points, no valid hypothesis) is a status code and the identity pose.
//
// gsr_pose_adam_update: the pose step of test_step_align (src/model/model_wrapper_style.py:430-440) for n views in one launch -- Adam
//   (torch.optim.Adam defaults, two parameter groups) on the zero deltas, then w2c' = SE3_exp(trans, rot) w2c
//   (src/misc/cam_utils.py:67-137), c2w' = w2c'^-1.
//
// (The SSIM structure term the refinement loop minimises is in gsr_ssim.hip.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

namespace gsr {
namespace pe {

// ======================================================================================================================
// PnP-RANSAC
// ======================================================================================================================
constexpr int PNP_SAMPLE = 6;                     // points per minimal sample (DLT)
constexpr int PNP_REFINE = 10;                    // fixed number of LM iterations
constexpr int PNP_GRANULE = 64;                   // points per mask granule (one ballot)
constexpr int PNP_THREADS = 256;
constexpr int PNP_PER_THREAD = 4;
constexpr int PNP_BLOCK_POINTS = PNP_THREADS * PNP_PER_THREAD;
constexpr int PNP_HCHUNK = 128;                   // hypotheses whose poses are in LDS at a time
constexpr int PNP_TERMS = 29;                     // 21 (upper triangle of J^T J) + 6 (J^T r) + truncated cost + inlier count
constexpr int PNP_TERMS_PAD = 32;
constexpr int PNP_STATE = 64;                     // doubles per problem: cur[12] cand[12] H[21] g[6] cost lambda
constexpr int ST_CUR = 0, ST_CAND = 12, ST_H = 24, ST_G = 45, ST_COST = 51, ST_LAMBDA = 52;
constexpr int PNP_MAX_ITER = 4096;

struct PnpLayout {
    size_t prefix, counts, valid, hypo, state, partial, total;
    int granules, blocks;
};

static PnpLayout pnp_layout(int64_t P, int64_t N, int iterations)
{
    PnpLayout L;
    L.granules = (int)((N + PNP_GRANULE - 1) / PNP_GRANULE);
    L.blocks = (int)((N + PNP_BLOCK_POINTS - 1) / PNP_BLOCK_POINTS);
    size_t o = 0;
    L.prefix = o; o = align_up(o + (size_t)P * (L.granules + 1) * sizeof(int32_t), 256);
    L.counts = o; o = align_up(o + (size_t)P * iterations * sizeof(int32_t), 256);
    L.valid = o; o = align_up(o + (size_t)P * iterations * sizeof(int32_t), 256);
    L.hypo = o; o = align_up(o + (size_t)P * iterations * 12 * sizeof(double), 256);
    L.state = o; o = align_up(o + (size_t)P * PNP_STATE * sizeof(double), 256);
    L.partial = o; o = align_up(o + (size_t)P * L.blocks * PNP_TERMS_PAD * sizeof(double), 256);
    L.total = o;
    return L;
}

struct PnpArgs {
    const float *pts, *opacity, *K;
    long long N;
    int W, iterations, granules, blocks;
    float opacity_threshold, reproj, pixel_offset;
    unsigned long long seed;
    int32_t *prefix, *counts, *valid, *status;
    double *hypo, *state, *partial;
    float *c2w;
    uint8_t *mask;
};

__device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;      // splitmix64's finaliser
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// r in [0, M): draw `d` of hypothesis `h`
__device__ inline unsigned int draw_index(unsigned long long seed, unsigned int h, unsigned int d, unsigned int M)
{
    const unsigned long long key = ((unsigned long long)h << 8) | d;
    const unsigned long long z = mix64(seed ^ mix64(key + 0x9E3779B97F4A7C15ull));
    return (unsigned int)(((z >> 32) * (unsigned long long)M) >> 32);
}

// ---- 1. mask counts per granule + exclusive prefix; zeroes the hypothesis counts and the status record ----
__global__ void __launch_bounds__(PNP_THREADS) k_pnp_prefix(PnpArgs a)
{
    __shared__ int seg[PNP_THREADS];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *op = a.opacity + (size_t)p * a.N;
    int32_t *prefix = a.prefix + (size_t)p * (a.granules + 1);
    for (int g = wave; g < a.granules; g += PNP_THREADS / 64) {
        const long long i = (long long)g * PNP_GRANULE + lane;
        const bool m = i < a.N && op[i] > a.opacity_threshold;
        const unsigned long long b = __ballot(m);
        if (lane == 0) prefix[g + 1] = __popcll(b);
    }
    for (int h = tid; h < a.iterations; h += PNP_THREADS) a.counts[(size_t)p * a.iterations + h] = 0;
    __syncthreads();
    // thread t owns granules [t per, (t + 1) per)
    const int per = (a.granules + PNP_THREADS - 1) / PNP_THREADS;
    const int g0 = min(tid * per, a.granules), g1 = min(g0 + per, a.granules);
    int s = 0;
    for (int g = g0; g < g1; ++g) s += prefix[g + 1];
    seg[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < PNP_THREADS; ++t) { const int v = seg[t]; seg[t] = run; run += v; }
        prefix[0] = 0;
        a.status[4 * p + 0] = run; a.status[4 * p + 1] = 0; a.status[4 * p + 2] = -1; a.status[4 * p + 3] = 0;
    }
    __syncthreads();
    int run = seg[tid];
    for (int g = g0; g < g1; ++g) { run += prefix[g + 1]; prefix[g + 1] = run; }   // prefix[g + 1] = masked points in granules 0..g
}

// ---- small float64 pose algebra (one thread) ----
struct Intr { double fx, sk, cx, fy, cy; };

__device__ inline Intr load_intr(const float *K)
{
    Intr k;
    k.fx = K[0]; k.sk = K[1]; k.cx = K[2]; k.fy = K[4]; k.cy = K[5];
    return k;
}

// adds one observation to acc[29]; returns whether the point is within the bound
__device__ inline bool accum_point(const double *R, const double *t, double X, double Y, double Z, double u, double v, const Intr &k,
                                   double bound2, double *acc)
{
    const double xc = R[0] * X + R[1] * Y + R[2] * Z + t[0];
    const double yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    const double zc = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    bool in = false;
    if (zc > 1e-9) {
        const double iz = 1.0 / zc;
        const double ru = (k.fx * xc + k.sk * yc) * iz + k.cx - u, rv = k.fy * yc * iz + k.cy - v;
        const double r2 = ru * ru + rv * rv;
        in = r2 <= bound2;
        if (in) {
            // d(proj)/d(x_c), then x_c' = x_c + rho + theta x x_c:  d x_c / d rho = I, d x_c / d theta = -[x_c]x
            const double a0 = k.fx * iz, a1 = k.sk * iz, a2 = -(k.fx * xc + k.sk * yc) * iz * iz;
            const double b1 = k.fy * iz, b2 = -k.fy * yc * iz * iz;
            const double J0[6] = {a0, a1, a2, a1 * (-zc) + a2 * yc, a0 * zc - a2 * xc, -a0 * yc + a1 * xc};
            const double J1[6] = {0.0, b1, b2, -b1 * zc + b2 * yc, -b2 * xc, b1 * xc};
            int q = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) acc[q++] += J0[i] * J0[j] + J1[i] * J1[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] += J0[i] * ru + J1[i] * rv;
            acc[27] += r2;
            acc[28] += 1.0;
            return true;
        }
    }
    acc[27] += bound2;                              // behind the camera, outside the bound or not finite: the truncated cost
    return false;
}

// (H + lambda diag(H)) d = -g by Gaussian elimination with partial pivoting; false if singular
__device__ inline bool solve6(const double *H21, const double *g, double lambda, double *d)
{
    double A[6][7];
    int q = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = H21[q]; A[j][i] = H21[q]; ++q; }
    for (int i = 0; i < 6; ++i) { A[i][i] += lambda * A[i][i] + 1e-300; A[i][6] = -g[i]; }
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        double best = fabs(A[c][c]);
        for (int r = c + 1; r < 6; ++r)
            if (fabs(A[r][c]) > best) { best = fabs(A[r][c]); piv = r; }
        if (!(best > 1e-200)) return false;
        if (piv != c)
            for (int j = 0; j < 7; ++j) { const double s = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = s; }
        const double inv = 1.0 / A[c][c];
        for (int r = c + 1; r < 6; ++r) {
            const double f = A[r][c] * inv;
            for (int j = c; j < 7; ++j) A[r][j] -= f * A[c][j];
        }
    }
    for (int r = 5; r >= 0; --r) {
        double s = A[r][6];
        for (int j = r + 1; j < 6; ++j) s -= A[r][j] * d[j];
        d[r] = s / A[r][r];
    }
    bool ok = true;
    for (int i = 0; i < 6; ++i) ok = ok && isfinite(d[i]);
    return ok;
}

// (R, t) <- SE3_exp(d) (R, t), d = (rho, theta) (src/misc/cam_utils.py:67-116, the angle < 1e-5 series included)
__device__ inline void se3_left(const double *d, const double *R, const double *t, double *Ro, double *to)
{
    const double th[3] = {d[3], d[4], d[5]}, rho[3] = {d[0], d[1], d[2]};
    const double Wm[3][3] = {{0.0, -th[2], th[1]}, {th[2], 0.0, -th[0]}, {-th[1], th[0], 0.0}};
    double W2[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W2[r][c] = Wm[r][0] * Wm[0][c] + Wm[r][1] * Wm[1][c] + Wm[r][2] * Wm[2][c];
    const double angle = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
    double rw, rw2, vw, vw2;
    if (angle < 1e-5) { rw = 1.0; rw2 = 0.5; vw = 0.5; vw2 = 1.0 / 6.0; }
    else {
        const double a2 = angle * angle;
        rw = sin(angle) / angle; rw2 = (1.0 - cos(angle)) / a2;
        vw = rw2; vw2 = (angle - sin(angle)) / (a2 * angle);
    }
    double E[3][3], tv[3];
    for (int r = 0; r < 3; ++r) {
        double s = 0.0;
        for (int c = 0; c < 3; ++c) {
            const double id = r == c ? 1.0 : 0.0;
            E[r][c] = id + rw * Wm[r][c] + rw2 * W2[r][c];
            s += (id + vw * Wm[r][c] + vw2 * W2[r][c]) * rho[c];
        }
        tv[r] = s;
    }
    double Rn[9], tn[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = E[r][0] * R[c] + E[r][1] * R[3 + c] + E[r][2] * R[6 + c];
        tn[r] = E[r][0] * t[0] + E[r][1] * t[1] + E[r][2] * t[2] + tv[r];
    }
    for (int i = 0; i < 9; ++i) Ro[i] = Rn[i];
    for (int i = 0; i < 3; ++i) to[i] = tn[i];
}

__device__ inline double det3(const double *A)
{
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// ---- 2. hypotheses ----
__global__ void __launch_bounds__(64) k_pnp_hypo(PnpArgs a)
{
    const int p = blockIdx.y;
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= a.iterations) return;
    const int M = a.status[4 * p + 0];
    int32_t *valid = a.valid + (size_t)p * a.iterations + h;
    double *out = a.hypo + ((size_t)p * a.iterations + h) * 12;
    *valid = 0;
    if (M < PNP_SAMPLE) return;
    const float *op = a.opacity + (size_t)p * a.N, *pts = a.pts + (size_t)p * a.N * 3;
    const int32_t *prefix = a.prefix + (size_t)p * (a.granules + 1);
    const Intr k = load_intr(a.K + 9 * (size_t)p);
    if (!(fabs(k.fx) > 1e-12 && fabs(k.fy) > 1e-12)) return;

    long long idx[PNP_SAMPLE];
    double X[PNP_SAMPLE][3], un[PNP_SAMPLE], vn[PNP_SAMPLE];
    for (int d = 0; d < PNP_SAMPLE; ++d) {
        const int r = (int)draw_index(a.seed, (unsigned)h, (unsigned)d, (unsigned)M);
        int lo = 0, hi = a.granules - 1;                              // largest g with prefix[g] <= r
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (prefix[mid] <= r) lo = mid; else hi = mid - 1;
        }
        int want = r - prefix[lo];
        const long long base = (long long)lo * PNP_GRANULE;
        unsigned long long bits = 0ull;
#pragma unroll 16
        for (int j = 0; j < PNP_GRANULE; ++j) {
            const long long i = base + j;
            const bool m = i < a.N && op[min(i, a.N - 1)] > a.opacity_threshold;
            bits |= (unsigned long long)m << j;
        }
        for (int s = 0; s < want; ++s) bits &= bits - 1;              // drop the `want` lowest set bits
        if (bits == 0ull) return;                                     // (cannot happen: the prefix counted the same mask)
        idx[d] = base + (__ffsll((long long)bits) - 1);
    }
    for (int d = 1; d < PNP_SAMPLE; ++d)
        for (int e = 0; e < d; ++e)
            if (idx[d] == idx[e]) return;                             // a repeated point
    double c[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < PNP_SAMPLE; ++d) {
        for (int q = 0; q < 3; ++q) { X[d][q] = (double)pts[3 * idx[d] + q]; c[q] += X[d][q] / PNP_SAMPLE; }
        const double px = (double)(idx[d] % a.W) + (double)a.pixel_offset, py = (double)(idx[d] / a.W) + (double)a.pixel_offset;
        vn[d] = (py - k.cy) / k.fy;
        un[d] = (px - k.cx - k.sk * vn[d]) / k.fx;
    }
    double s2 = 0.0;
    for (int d = 0; d < PNP_SAMPLE; ++d)
        for (int q = 0; q < 3; ++q) { const double e = X[d][q] - c[q]; s2 += e * e; }
    const double sc = sqrt(s2 / PNP_SAMPLE);
    if (!(sc > 1e-12) || !isfinite(sc)) return;
    // DLT with p34 = 1: unknowns (p1[4], p2[4], p3[3]); rows u: [Xh 0 -u X | u], v: [0 Xh -v X | v]; the last v row is left out
    double A[11][12];
    for (int r = 0; r < 11; ++r) {
        const int d = r >> 1;
        const bool isv = r & 1;
        const double x0 = (X[d][0] - c[0]) / sc, x1 = (X[d][1] - c[1]) / sc, x2 = (X[d][2] - c[2]) / sc;
        const double o = isv ? vn[d] : un[d];
        for (int j = 0; j < 12; ++j) A[r][j] = 0.0;
        const int b = isv ? 4 : 0;
        A[r][b] = x0; A[r][b + 1] = x1; A[r][b + 2] = x2; A[r][b + 3] = 1.0;
        A[r][8] = -o * x0; A[r][9] = -o * x1; A[r][10] = -o * x2;
        A[r][11] = o;
    }
    for (int col = 0; col < 11; ++col) {
        int piv = col;
        double best = fabs(A[col][col]);
        for (int r = col + 1; r < 11; ++r)
            if (fabs(A[r][col]) > best) { best = fabs(A[r][col]); piv = r; }
        if (!(best > 1e-9)) return;                                   // (near-)degenerate sample: collinear / coplanar points
        if (piv != col)
            for (int j = 0; j < 12; ++j) { const double s = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = s; }
        const double inv = 1.0 / A[col][col];
        for (int r = col + 1; r < 11; ++r) {
            const double f = A[r][col] * inv;
            for (int j = col; j < 12; ++j) A[r][j] -= f * A[col][j];
        }
    }
    double th[11];
    for (int r = 10; r >= 0; --r) {
        double s = A[r][11];
        for (int j = r + 1; j < 11; ++j) s -= A[r][j] * th[j];
        th[r] = s / A[r][r];
    }
    // x_cam ~ M' (X - c) / sc + p4' = Am X + bv
    double Am[9] = {th[0] / sc, th[1] / sc, th[2] / sc, th[4] / sc, th[5] / sc, th[6] / sc, th[8] / sc, th[9] / sc, th[10] / sc};
    double bv[3] = {th[3], th[7], 1.0};
    for (int r = 0; r < 3; ++r) bv[r] -= Am[3 * r] * c[0] + Am[3 * r + 1] * c[1] + Am[3 * r + 2] * c[2];
    const double det = det3(Am);
    if (!(det > 1e-300) || !isfinite(det)) return;                    // a reflection: the sample's centroid behind the camera
    const double mu = 1.0 / cbrt(det);
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = mu * Am[i];
    for (int i = 0; i < 3; ++i) t[i] = mu * bv[i];
    for (int it = 0; it < 12; ++it) {                                 // polar factor: R <- (R + R^-T) / 2
        const double dt = det3(R);
        if (!(fabs(dt) > 1e-12)) return;
        const double C[9] = {R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6],
                             R[2] * R[7] - R[1] * R[8], R[0] * R[8] - R[2] * R[6], R[1] * R[6] - R[0] * R[7],
                             R[1] * R[5] - R[2] * R[4], R[2] * R[3] - R[0] * R[5], R[0] * R[4] - R[1] * R[3]};   // cofactors = det R^-T
        for (int i = 0; i < 9; ++i) R[i] = 0.5 * (R[i] + C[i] / dt);
    }
    // Gauss-Newton on the six reprojection errors (normalised image coordinates)
    const Intr unit = {1.0, 0.0, 0.0, 1.0, 0.0};
    for (int it = 0; it < 5; ++it) {
        double acc[PNP_TERMS];
        for (int i = 0; i < PNP_TERMS; ++i) acc[i] = 0.0;
        for (int d = 0; d < PNP_SAMPLE; ++d) accum_point(R, t, X[d][0], X[d][1], X[d][2], un[d], vn[d], unit, 1e300, acc);
        double dl[6];
        if (acc[28] < PNP_SAMPLE || !solve6(acc, acc + 21, 1e-9, dl)) return;
        se3_left(dl, R, t, R, t);
    }
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(R[i]);
    for (int i = 0; i < 3; ++i) ok = ok && isfinite(t[i]);
    for (int d = 0; d < PNP_SAMPLE; ++d) ok = ok && (R[6] * X[d][0] + R[7] * X[d][1] + R[8] * X[d][2] + t[2] > 1e-9);
    if (!ok) return;
    for (int i = 0; i < 9; ++i) out[i] = R[i];
    for (int i = 0; i < 3; ++i) out[9 + i] = t[i];
    *valid = 1;
}

// ---- 3. scoring ----
__global__ void __launch_bounds__(PNP_THREADS) k_pnp_score(PnpArgs a)
{
    __shared__ float pose[PNP_HCHUNK][12];
    __shared__ int ok[PNP_HCHUNK];
    __shared__ int cnt[PNP_HCHUNK];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    if (a.status[4 * p + 0] < PNP_SAMPLE) return;
    const float *op = a.opacity + (size_t)p * a.N, *pts = a.pts + (size_t)p * a.N * 3;
    const float *K = a.K + 9 * (size_t)p;
    const float fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
    const float bound2 = a.reproj * a.reproj;
    float X[PNP_PER_THREAD], Y[PNP_PER_THREAD], Z[PNP_PER_THREAD], U[PNP_PER_THREAD], V[PNP_PER_THREAD];
    bool m[PNP_PER_THREAD];
#pragma unroll
    for (int q = 0; q < PNP_PER_THREAD; ++q) {
        const long long i = (long long)blockIdx.x * PNP_BLOCK_POINTS + q * PNP_THREADS + tid;
        m[q] = i < a.N && op[i] > a.opacity_threshold;
        X[q] = Y[q] = Z[q] = U[q] = V[q] = 0.f;
        if (m[q]) {
            X[q] = pts[3 * i]; Y[q] = pts[3 * i + 1]; Z[q] = pts[3 * i + 2];
            U[q] = (float)(i % a.W) + a.pixel_offset; V[q] = (float)(i / a.W) + a.pixel_offset;
        }
    }
    for (int h0 = 0; h0 < a.iterations; h0 += PNP_HCHUNK) {
        const int nh = min(PNP_HCHUNK, a.iterations - h0);
        __syncthreads();
        for (int e = tid; e < nh * 12; e += PNP_THREADS)
            pose[e / 12][e % 12] = (float)a.hypo[((size_t)p * a.iterations + h0) * 12 + e];
        for (int e = tid; e < nh; e += PNP_THREADS) { ok[e] = a.valid[(size_t)p * a.iterations + h0 + e]; cnt[e] = 0; }
        __syncthreads();
        for (int h = 0; h < nh; ++h) {
            if (!ok[h]) continue;                                      // (block-uniform)
            const float *T = pose[h];
            int c = 0;
#pragma unroll
            for (int q = 0; q < PNP_PER_THREAD; ++q) {
                const float xc = T[0] * X[q] + T[1] * Y[q] + T[2] * Z[q] + T[9];
                const float yc = T[3] * X[q] + T[4] * Y[q] + T[5] * Z[q] + T[10];
                const float zc = T[6] * X[q] + T[7] * Y[q] + T[8] * Z[q] + T[11];
                const float iz = 1.f / zc;
                const float du = (fx * xc + sk * yc) * iz + cx - U[q], dv = fy * yc * iz + cy - V[q];
                const bool in = m[q] && zc > 1e-6f && du * du + dv * dv <= bound2;
                c += __popcll(__ballot(in));
            }
            if (lane == 0 && c) atomicAdd(&cnt[h], c);
        }
        __syncthreads();
        for (int e = tid; e < nh; e += PNP_THREADS)
            if (cnt[e]) atomicAdd(&a.counts[(size_t)p * a.iterations + h0 + e], cnt[e]);
    }
}

// ---- 4. the winner ----
__global__ void __launch_bounds__(64) k_pnp_select(PnpArgs a, int P)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int M = a.status[4 * p + 0];
    int best = -1, bc = -1;
    for (int h = 0; h < a.iterations; ++h) {
        if (!a.valid[(size_t)p * a.iterations + h]) continue;
        const int c = a.counts[(size_t)p * a.iterations + h];
        if (c > bc) { bc = c; best = h; }                              // strict: ties stay with the lowest index
    }
    double *st = a.state + (size_t)p * PNP_STATE;
    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    int code = 0;
    if (M < PNP_SAMPLE) code = 1;
    else if (best < 0 || bc < PNP_SAMPLE) code = 2;
    for (int i = 0; i < 12; ++i) {
        const double v = code ? I[i] : a.hypo[((size_t)p * a.iterations + best) * 12 + i];
        st[ST_CUR + i] = v; st[ST_CAND + i] = v;
    }
    for (int i = 0; i < 27; ++i) st[ST_H + i] = 0.0;
    st[ST_COST] = 1e300;
    st[ST_LAMBDA] = 1e-3;
    a.status[4 * p + 2] = code ? -1 : best;
    a.status[4 * p + 3] = code;
}

// ---- 5a. normal equations and truncated cost of the candidate pose, per block ----
__global__ void __launch_bounds__(PNP_THREADS) k_pnp_accum(PnpArgs a)
{
    __shared__ double red[PNP_THREADS / 64][PNP_TERMS_PAD];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.status[4 * p + 3] != 0) return;
    const float *op = a.opacity + (size_t)p * a.N, *pts = a.pts + (size_t)p * a.N * 3;
    const Intr k = load_intr(a.K + 9 * (size_t)p);
    const double *st = a.state + (size_t)p * PNP_STATE + ST_CAND;
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = st[i];
    for (int i = 0; i < 3; ++i) t[i] = st[9 + i];
    const double bound2 = (double)a.reproj * (double)a.reproj;
    double acc[PNP_TERMS];
#pragma unroll
    for (int i = 0; i < PNP_TERMS; ++i) acc[i] = 0.0;
#pragma unroll
    for (int q = 0; q < PNP_PER_THREAD; ++q) {
        const long long i = (long long)blockIdx.x * PNP_BLOCK_POINTS + q * PNP_THREADS + tid;
        if (i < a.N && op[i] > a.opacity_threshold)
            accum_point(R, t, (double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2], (double)(i % a.W) + (double)a.pixel_offset,
                        (double)(i / a.W) + (double)a.pixel_offset, k, bound2, acc);
    }
#pragma unroll
    for (int i = 0; i < PNP_TERMS; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (tid < PNP_TERMS) {
        double s = 0.0;
        for (int w = 0; w < PNP_THREADS / 64; ++w) s += red[w][tid];
        a.partial[((size_t)p * a.blocks + blockIdx.x) * PNP_TERMS_PAD + tid] = s;
    }
}

// ---- 5b. fold in block order, accept / reject, next candidate ----
__global__ void __launch_bounds__(64) k_pnp_step(PnpArgs a, int last)
{
    __shared__ double f[PNP_TERMS_PAD];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (a.status[4 * p + 3] != 0) return;
    if (lane < PNP_TERMS) {
        double s = 0.0;
        for (int b = 0; b < a.blocks; ++b) s += a.partial[((size_t)p * a.blocks + b) * PNP_TERMS_PAD + lane];
        f[lane] = s;
    }
    __syncthreads();
    if (lane != 0) return;
    double *st = a.state + (size_t)p * PNP_STATE;
    double lambda = st[ST_LAMBDA];
    if (f[27] < st[ST_COST] && f[28] >= PNP_SAMPLE) {
        for (int i = 0; i < 12; ++i) st[ST_CUR + i] = st[ST_CAND + i];
        for (int i = 0; i < 27; ++i) st[ST_H + i] = f[i];
        st[ST_COST] = f[27];
        lambda = fmax(lambda * 0.2, 1e-12);
    } else {
        lambda = fmin(lambda * 10.0, 1e12);
    }
    st[ST_LAMBDA] = lambda;
    if (last) return;
    double d[6];
    if (solve6(st + ST_H, st + ST_G, lambda, d)) se3_left(d, st + ST_CUR, st + ST_CUR + 9, st + ST_CAND, st + ST_CAND + 9);
    else for (int i = 0; i < 12; ++i) st[ST_CAND + i] = st[ST_CUR + i];
}

// ---- 6. mask, count, c2w ----
__global__ void __launch_bounds__(PNP_THREADS) k_pnp_finish(PnpArgs a)
{
    __shared__ int red[PNP_THREADS / 64];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool failed = a.status[4 * p + 3] != 0;
    const float *op = a.opacity + (size_t)p * a.N, *pts = a.pts + (size_t)p * a.N * 3;
    const Intr k = load_intr(a.K + 9 * (size_t)p);
    const double *st = a.state + (size_t)p * PNP_STATE + ST_CUR;
    double R[9], t[3];
    for (int i = 0; i < 9; ++i) R[i] = st[i];
    for (int i = 0; i < 3; ++i) t[i] = st[9 + i];
    const double bound2 = (double)a.reproj * (double)a.reproj;
    int c = 0;
#pragma unroll
    for (int q = 0; q < PNP_PER_THREAD; ++q) {
        const long long i = (long long)blockIdx.x * PNP_BLOCK_POINTS + q * PNP_THREADS + tid;
        bool in = false;
        if (!failed && i < a.N && op[i] > a.opacity_threshold) {
            const double X = pts[3 * i], Y = pts[3 * i + 1], Z = pts[3 * i + 2];
            const double xc = R[0] * X + R[1] * Y + R[2] * Z + t[0], yc = R[3] * X + R[4] * Y + R[5] * Z + t[1];
            const double zc = R[6] * X + R[7] * Y + R[8] * Z + t[2];
            if (zc > 1e-9) {
                const double iz = 1.0 / zc;
                const double ru = (k.fx * xc + k.sk * yc) * iz + k.cx - ((double)(i % a.W) + (double)a.pixel_offset);
                const double rv = k.fy * yc * iz + k.cy - ((double)(i / a.W) + (double)a.pixel_offset);
                in = ru * ru + rv * rv <= bound2;
            }
        }
        if (a.mask && i < a.N) a.mask[(size_t)p * a.N + i] = in ? 1 : 0;
        c += __popcll(__ballot(in));
    }
    if (lane == 0) red[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < PNP_THREADS / 64; ++w) s += red[w];
        if (s) atomicAdd(&a.status[4 * p + 1], s);
        if (blockIdx.x == 0) {
            // c2w = (R | t)^-1 = (R^T | -R^T t)
            float *o = a.c2w + 16 * (size_t)p;
            for (int r = 0; r < 3; ++r) {
                for (int cc = 0; cc < 3; ++cc) o[4 * r + cc] = (float)R[3 * cc + r];
                o[4 * r + 3] = (float)-(R[r] * t[0] + R[3 + r] * t[1] + R[6 + r] * t[2]);
            }
            o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
        }
    }
}

// ======================================================================================================================
// Pose step: one thread per view
// ======================================================================================================================
__device__ inline void inverse4_f64(const double *m, double *inv)
{
    // Gauss-Jordan with partial pivoting on [m | I] (row-major): the general inverse of update_pose's `extrinsics.inverse()`
    double a[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { a[r][c] = m[4 * r + c]; a[r][4 + c] = (r == c) ? 1.0 : 0.0; }
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        double best = fabs(a[col][col]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r > col && fabs(a[r][col]) > best) { best = fabs(a[r][col]); piv = r; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r == piv && piv != col) {
#pragma unroll
                for (int c = 0; c < 8; ++c) { const double t = a[col][c]; a[col][c] = a[r][c]; a[r][c] = t; }
            }
        const double d = 1.0 / a[col][col];
#pragma unroll
        for (int c = 0; c < 8; ++c) a[col][c] *= d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
#pragma unroll
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) inv[4 * r + c] = a[r][4 + c];
}

__global__ void __launch_bounds__(64) k_pose_adam(float *__restrict__ c2w, float *__restrict__ m, float *__restrict__ v,
                                                  const float *__restrict__ grad_rot, const float *__restrict__ grad_trans, long long n,
                                                  float step_rot, float step_trans, float beta1, float beta2, float eps, float bc2_sqrt)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // Adam on a parameter that is 0 before every step (the reference resets the deltas): theta = -step_size * m / denom, with
    // torch's fp32 arithmetic (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), sqrt / bc2_sqrt + eps, addcdiv_)
    double d[6];                                   // (rot, trans) -> tau = (rho = trans, theta = rot) below
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const float g = q < 3 ? grad_rot[3 * i + q] : grad_trans[3 * i + q - 3];
        float mq = m[6 * i + q], vq = v[6 * i + q];
        mq = mq + (1.f - beta1) * (g - mq);
        vq = vq * beta2 + (1.f - beta2) * g * g;
        m[6 * i + q] = mq; v[6 * i + q] = vq;
        const float denom = sqrtf(vq) / bc2_sqrt + eps;
        d[q] = (double)(-(q < 3 ? step_rot : step_trans) * (mq / denom));
    }
    const double th[3] = {d[0], d[1], d[2]}, rho[3] = {d[3], d[4], d[5]};
    // SE3_exp (cam_utils.py:67-116): W = [theta]x, R = SO3_exp(theta), t = V(theta) rho
    const double Wm[3][3] = {{0.0, -th[2], th[1]}, {th[2], 0.0, -th[0]}, {-th[1], th[0], 0.0}};
    double W2[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W2[r][c] = Wm[r][0] * Wm[0][c] + Wm[r][1] * Wm[1][c] + Wm[r][2] * Wm[2][c];
    const double angle = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
    double rw, rw2, vw, vw2;
    if (angle < 1e-5) { rw = 1.0; rw2 = 0.5; vw = 0.5; vw2 = 1.0 / 6.0; }
    else {
        const double a2 = angle * angle;
        rw = sin(angle) / angle; rw2 = (1.0 - cos(angle)) / a2;
        vw = rw2; vw2 = (angle - sin(angle)) / (a2 * angle);
    }
    double T[16];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double id = r == c ? 1.0 : 0.0;
            T[4 * r + c] = id + rw * Wm[r][c] + rw2 * W2[r][c];
            t += (id + vw * Wm[r][c] + vw2 * W2[r][c]) * rho[c];
        }
        T[4 * r + 3] = t;
    }
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
    double E[16], w2c[16], nw[16], out[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) E[q] = (double)c2w[16 * i + q];
    inverse4_f64(E, w2c);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            nw[4 * r + c] = T[4 * r] * w2c[c] + T[4 * r + 1] * w2c[4 + c] + T[4 * r + 2] * w2c[8 + c] + T[4 * r + 3] * w2c[12 + c];
    inverse4_f64(nw, out);
#pragma unroll
    for (int q = 0; q < 16; ++q) c2w[16 * i + q] = (float)out[q];
}

}  // namespace pe
}  // namespace gsr

extern "C" {

using namespace gsr::pe;

__attribute__((visibility("default"))) size_t gsr_pnp_ransac_scratch_bytes(int64_t P, int H, int W, int iterations)
{
    if (P < 1 || P > 65535 || H < 1 || W < 1 || iterations < 1 || iterations > PNP_MAX_ITER) return 0;
    return pnp_layout(P, (int64_t)H * W, iterations).total;
}

__attribute__((visibility("default"))) int gsr_pnp_ransac(const float *pts3d, const float *opacity, const float *K, int64_t P, int H, int W,
                                                          int64_t N, float opacity_threshold, float reprojection_error, int iterations,
                                                          uint64_t seed, float pixel_offset, float *c2w, uint8_t *inlier_mask, int32_t *status,
                                                          void *scratch, void *stream)
{
    if (!pts3d || !opacity || !K || !c2w || !status || !scratch) return GSR_EINVAL;
    if (P < 1 || P > 65535 || H < 1 || W < 1 || N != (int64_t)H * W || N > 0x3fffffffLL || iterations < 1 || iterations > PNP_MAX_ITER)
        return GSR_EINVAL;
    if (!(reprojection_error > 0.f) || !isfinite(opacity_threshold) || !isfinite(pixel_offset)) return GSR_EINVAL;
    const PnpLayout L = pnp_layout(P, N, iterations);
    char *base = static_cast<char *>(scratch);
    PnpArgs a;
    a.pts = pts3d; a.opacity = opacity; a.K = K;
    a.N = N; a.W = W; a.iterations = iterations; a.granules = L.granules; a.blocks = L.blocks;
    a.opacity_threshold = opacity_threshold; a.reproj = reprojection_error; a.pixel_offset = pixel_offset;
    a.seed = seed;
    a.prefix = reinterpret_cast<int32_t *>(base + L.prefix); a.counts = reinterpret_cast<int32_t *>(base + L.counts);
    a.valid = reinterpret_cast<int32_t *>(base + L.valid); a.status = status;
    a.hypo = reinterpret_cast<double *>(base + L.hypo); a.state = reinterpret_cast<double *>(base + L.state);
    a.partial = reinterpret_cast<double *>(base + L.partial);
    a.c2w = c2w; a.mask = inlier_mask;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 pts_grid((unsigned)L.blocks, (unsigned)P);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pnp_prefix, dim3((unsigned)P), dim3(PNP_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_pnp_hypo, dim3((unsigned)((iterations + 63) / 64), (unsigned)P), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_pnp_score, pts_grid, dim3(PNP_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_pnp_select, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, st, a, (int)P);
    for (int it = 0; it < PNP_REFINE; ++it) {
        hipLaunchKernelGGL(k_pnp_accum, pts_grid, dim3(PNP_THREADS), 0, st, a);
        hipLaunchKernelGGL(k_pnp_step, dim3((unsigned)P), dim3(64), 0, st, a, it == PNP_REFINE - 1 ? 1 : 0);
    }
    hipLaunchKernelGGL(k_pnp_finish, pts_grid, dim3(PNP_THREADS), 0, st, a);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) int gsr_pose_adam_update(float *c2w, float *m, float *v, const float *grad_rot, const float *grad_trans,
                                                                int64_t n, int step, float lr_rot, float lr_trans, float beta1, float beta2,
                                                                float eps, void *stream)
{
    if (!c2w || !m || !v || !grad_rot || !grad_trans || n < 1 || step < 1) return GSR_EINVAL;
    // torch.optim.Adam (capturable=False): the bias corrections and the step size are host doubles, used by the fp32 kernel as floats
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pose_adam, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), c2w, m, v, grad_rot,
                       grad_trans, (long long)n, (float)(lr_rot / bc1), (float)(lr_trans / bc1), beta1, beta2, eps, (float)sqrt(bc2));
    return gsr::launch_status();
}

}  // extern "C"
