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
// gsr_ssim_structure_fwd / _bwd: `1 - structure` of src/loss/loss_ssim.py:80-124 (data_range 1, K = (0.01, 0.03), valid 11 x 11 window,
//   compensation 1, eps^2 / min / 0.98 clamps) with the tiling of k_image_scores (gsr_metrics.hip): one wave per (plane, strip of 64 columns,
//   chunk of 32 rows), rows staged through LDS, an 11-row register ring, moments of the images shifted by the tile's first pixel (summed in
//   float64, kept in fp32; the window's sum differs from 1 in fp32 and the shift is corrected for it).  The
//   forward optionally leaves the three per-pixel adjoint maps (d/d mu2, d/d E[y^2], d/d E[xy]); the backward is the same walk over those
//   maps, zero-padded by 10 on every side (the transposed filter), combined with the pixel's own x and y.
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

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static PnpLayout pnp_layout(int64_t P, int64_t N, int iterations)
{
    PnpLayout L;
    L.granules = (int)((N + PNP_GRANULE - 1) / PNP_GRANULE);
    L.blocks = (int)((N + PNP_BLOCK_POINTS - 1) / PNP_BLOCK_POINTS);
    size_t o = 0;
    L.prefix = o; o = align256(o + (size_t)P * (L.granules + 1) * sizeof(int32_t));
    L.counts = o; o = align256(o + (size_t)P * iterations * sizeof(int32_t));
    L.valid = o; o = align256(o + (size_t)P * iterations * sizeof(int32_t));
    L.hypo = o; o = align256(o + (size_t)P * iterations * 12 * sizeof(double));
    L.state = o; o = align256(o + (size_t)P * PNP_STATE * sizeof(double));
    L.partial = o; o = align256(o + (size_t)P * L.blocks * PNP_TERMS_PAD * sizeof(double));
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

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
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
// SSIM structure term
// ======================================================================================================================
constexpr int SS_COLS = 64;
constexpr int SS_ROWS = 32;
constexpr int SS_R = 5;
constexpr int SS_WIN = 2 * SS_R + 1;
constexpr int SS_IN = SS_COLS + 2 * SS_R;
constexpr float SS_C3 = 0.5f * (0.03f * 0.03f);                       // C2 / 2, C2 = (K2 data_range)^2
constexpr float SS_EPS2 = 1.1920928955078125e-07f * 1.1920928955078125e-07f;   // finfo(float32).eps^2
constexpr float SS_CLAMP = 0.98f;

struct Window {
    float w[SS_WIN];
};

__global__ void __launch_bounds__(64) k_ssim_struct_fwd(const float *__restrict__ gt, const float *__restrict__ pred, int H, int W, int strips,
                                                        int chunks, Window win, double wsum2, double *__restrict__ partial,
                                                        float *__restrict__ maps, size_t map_stride)
{
    __shared__ float sx[2][SS_IN], sy[2][SS_IN];
    const int lane = threadIdx.x;
    const int tiles = strips * chunks;
    const long long blk = blockIdx.x;
    const long long plane = blk / tiles;
    const int t = (int)(blk - plane * tiles);
    const int k = t / strips, s = t - k * strips;
    const int Ho = H - 2 * SS_R, Wo = W - 2 * SS_R;
    const int c0 = s * SS_COLS;
    const int r0 = k * SS_ROWS, r1 = min(r0 + SS_ROWS, Ho) + 2 * SS_R;    // input rows [r0, r1)
    const float *X = gt + (size_t)plane * H * W, *Y = pred + (size_t)plane * H * W;
    const float kx = X[(size_t)r0 * W + c0], ky = Y[(size_t)r0 * W + c0];
    const int cm = c0 + lane, ch = c0 + SS_COLS + lane;
    const bool in_m = cm < W, in_h = lane < 2 * SS_R && ch < W;
    const bool out_col = cm < Wo;

    float xm = 0.f, ym = 0.f, xh = 0.f, yh = 0.f;
    auto load_row = [&](int r) {
        const size_t o = (size_t)r * W;
        xm = in_m ? X[o + cm] : 0.f; ym = in_m ? Y[o + cm] : 0.f;
        xh = in_h ? X[o + ch] : 0.f; yh = in_h ? Y[o + ch] : 0.f;
    };
    load_row(r0);

    float ring[SS_WIN][5];
    double acc = 0.0;
    for (int rb = r0; rb < r1; rb += SS_WIN) {
#pragma unroll
        for (int j = 0; j < SS_WIN; ++j) {
            const int r = rb + j;
            if (r >= r1) continue;
            const int b = (r - r0) & 1;
            sx[b][lane] = xm - kx; sy[b][lane] = ym - ky;
            if (lane < 2 * SS_R) { sx[b][SS_COLS + lane] = xh - kx; sy[b][SS_COLS + lane] = yh - ky; }
            if (r + 1 < r1) load_row(r + 1);
            __syncthreads();
            // float64 sums (the products of fp32 values are exact in it), fp32 ring: the variances are differences of these sums
            double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
            for (int q = 0; q < SS_WIN; ++q) {
                const double av = (double)sx[b][lane + q], cv = (double)sy[b][lane + q], wa = (double)win.w[q] * av, wc = (double)win.w[q] * cv;
                h0 += wa; h1 += wc; h2 += wa * av; h3 += wc * cv; h4 += wa * cv;
            }
            ring[j][0] = (float)h0; ring[j][1] = (float)h1; ring[j][2] = (float)h2; ring[j][3] = (float)h3; ring[j][4] = (float)h4;
            if (r - r0 >= 2 * SS_R && out_col) {
                double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
                for (int i = 0; i < SS_WIN; ++i) {
                    const int sl = (j + 1 + i) % SS_WIN;
                    const double w = (double)win.w[i];
                    m0 += w * (double)ring[sl][0]; m1 += w * (double)ring[sl][1]; m2 += w * (double)ring[sl][2];
                    m3 += w * (double)ring[sl][3]; m4 += w * (double)ring[sl][4];
                }
                // The fp32-normalised taps do not sum to 1 exactly (wsum2 = (sum w)^2 over the 11 x 11 window), so variances are NOT
                // invariant under the shift: sum w x^2 - (sum w x)^2 = m2 - m0^2 + (1 - wsum2) (2 kx m0 + kx^2 wsum2) for x = a + kx.
                const double oms = 1.0 - wsum2, dkx = (double)kx, dky = (double)ky;
                const float s1 = (float)(m2 - m0 * m0 + oms * (2.0 * dkx * m0 + dkx * dkx * wsum2));
                const float s2 = (float)(m3 - m1 * m1 + oms * (2.0 * dky * m1 + dky * dky * wsum2));
                const float c = (float)(m4 - m0 * m1 + oms * (dkx * m1 + dky * m0 + dkx * dky * wsum2));
                const float ux = (float)(m0 + dkx * wsum2), uy = (float)(m1 + dky * wsum2);      // sum w x, sum w y
                const float v1 = fmaxf(s1, SS_EPS2), v2 = fmaxf(s2, SS_EPS2);
                const float pr = sqrtf(v1 * v2), ac = fabsf(c);
                const bool capped = ac > pr;
                const float cp = capped ? copysignf(pr, c) : c;
                const float q1 = sqrtf(v1), q2 = sqrtf(v2);
                const float D = q1 * q2 + SS_C3;
                const float sv = (cp + SS_C3) / D;
                const bool clamped = sv > SS_CLAMP;
                acc += (double)(clamped ? SS_CLAMP : sv);
                if (maps) {
                    float a_mu = 0.f, a_yy = 0.f, a_c = 0.f;
                    if (!clamped) {
                        const float invD = 1.f / D;
                        a_c = capped ? 0.f : invD;
                        float dv2 = -(sv * invD) * (q1 / (2.f * q2));
                        if (capped) dv2 += copysignf(invD, c) * (v1 / (2.f * pr));
                        a_yy = (s2 < SS_EPS2) ? 0.f : dv2;
                        a_mu = -2.f * uy * a_yy - ux * a_c;
                    }
                    const size_t o = ((size_t)plane * Ho + (r - 2 * SS_R)) * Wo + cm;
                    maps[o] = a_mu; maps[map_stride + o] = a_yy; maps[2 * map_stride + o] = a_c;
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) partial[blk] = acc;
}

// one wave per image: its C * tiles partials in index order
__global__ void __launch_bounds__(64) k_ssim_struct_fold(const double *__restrict__ partial, int per_image, double inv, float *__restrict__ out)
{
    const long long n = blockIdx.x;
    const double *p = partial + n * per_image;
    double s = 0.0;
    for (int i = threadIdx.x; i < per_image; i += 64) s += p[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) out[n] = (float)(s * inv);
}

// one wave per (plane, strip of 64 image columns, chunk of 32 image rows): the valid filter of the adjoint maps padded with 10 zeros
__global__ void __launch_bounds__(64) k_ssim_struct_bwd(const float *__restrict__ gt, const float *__restrict__ pred,
                                                        const float *__restrict__ maps, size_t map_stride, const float *__restrict__ grad_out,
                                                        float inv_norm, int C, int H, int W, int strips, int chunks, Window win,
                                                        float *__restrict__ grad)
{
    __shared__ float sm[2][3][SS_IN];
    const int lane = threadIdx.x;
    const int tiles = strips * chunks;
    const long long blk = blockIdx.x;
    const long long plane = blk / tiles;
    const int t = (int)(blk - plane * tiles);
    const int k = t / strips, s = t - k * strips;
    const int Ho = H - 2 * SS_R, Wo = W - 2 * SS_R;
    const int c0 = s * SS_COLS;
    const int r0 = k * SS_ROWS, r1 = min(r0 + SS_ROWS, H);                 // image rows [r0, r1)
    const int m0 = r0 - 2 * SS_R;                                          // first (virtual) map row of the walk
    const float *X = gt + (size_t)plane * H * W, *Y = pred + (size_t)plane * H * W;
    const float *A0 = maps + (size_t)plane * Ho * Wo, *A1 = A0 + map_stride, *A2 = A1 + map_stride;
    const float scale = grad_out[plane / C] * inv_norm;
    const int mc = c0 - 2 * SS_R + lane, hc = c0 + SS_COLS - 2 * SS_R + lane;
    const bool in_m = mc >= 0 && mc < Wo, in_h = lane < 2 * SS_R && hc < Wo;
    const int ci = c0 + lane;

    float am[3] = {0.f, 0.f, 0.f}, ah[3] = {0.f, 0.f, 0.f};
    auto load_row = [&](int m) {
        const bool row = m >= 0 && m < Ho;                                  // (uniform)
        const size_t o = (size_t)(row ? m : 0) * Wo;
        am[0] = row && in_m ? A0[o + mc] : 0.f; am[1] = row && in_m ? A1[o + mc] : 0.f; am[2] = row && in_m ? A2[o + mc] : 0.f;
        ah[0] = row && in_h ? A0[o + hc] : 0.f; ah[1] = row && in_h ? A1[o + hc] : 0.f; ah[2] = row && in_h ? A2[o + hc] : 0.f;
    };
    load_row(m0);

    float ring[SS_WIN][3];
    for (int mb = m0; mb < r1; mb += SS_WIN) {
#pragma unroll
        for (int j = 0; j < SS_WIN; ++j) {
            const int m = mb + j;
            if (m >= r1) continue;
            const int b = (m - m0) & 1;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                sm[b][q][lane] = am[q];
                if (lane < 2 * SS_R) sm[b][q][SS_COLS + lane] = ah[q];
            }
            if (m + 1 < r1) load_row(m + 1);
            __syncthreads();
            float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
            for (int q = 0; q < SS_WIN; ++q) {
                const float w = win.w[SS_WIN - 1 - q];
                h0 += w * sm[b][0][lane + q]; h1 += w * sm[b][1][lane + q]; h2 += w * sm[b][2][lane + q];
            }
            ring[j][0] = h0; ring[j][1] = h1; ring[j][2] = h2;
            if (m >= r0 && ci < W) {                                        // map rows m-10 .. m are in slots j+1 .. j (mod 11)
                float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
                for (int i = 0; i < SS_WIN; ++i) {
                    const int sl = (j + 1 + i) % SS_WIN;
                    const float w = win.w[SS_WIN - 1 - i];
                    v0 += w * ring[sl][0]; v1 += w * ring[sl][1]; v2 += w * ring[sl][2];
                }
                const size_t o = (size_t)m * W + ci;
                grad[(size_t)plane * H * W + o] = scale * (v0 + 2.f * Y[o] * v1 + X[o] * v2);
            }
        }
    }
}

static bool ssim_grid(int64_t N, int C, int H, int W, bool image_rows, int &strips, int &chunks, long long &blocks)
{
    if (N < 1 || C < 1 || H < SS_WIN || W < SS_WIN) return false;
    const int cols = image_rows ? W : W - 2 * SS_R, rows = image_rows ? H : H - 2 * SS_R;
    strips = (cols + SS_COLS - 1) / SS_COLS;
    chunks = (rows + SS_ROWS - 1) / SS_ROWS;
    blocks = (long long)N * C * strips * chunks;
    return blocks <= 0x7fffffffLL && (long long)N * C * H * W <= 0x7fffffffffLL;
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

__attribute__((visibility("default"))) size_t gsr_ssim_structure_scratch_bytes(int64_t N, int C, int H, int W)
{
    int strips, chunks;
    long long blocks;
    if (!ssim_grid(N, C, H, W, false, strips, chunks, blocks)) return 0;
    return (size_t)blocks * sizeof(double);
}

__attribute__((visibility("default"))) int gsr_ssim_structure_fwd(const float *target, const float *pred, int64_t N, int C, int H, int W,
                                                                  const float *window, float *structure, float *maps, void *scratch,
                                                                  void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!target || !pred || !window || !structure || !scratch || !ssim_grid(N, C, H, W, false, strips, chunks, blocks)) return GSR_EINVAL;
    Window win;
    double wsum = 0.0;
    for (int q = 0; q < SS_WIN; ++q) { win.w[q] = window[q]; wsum += (double)window[q]; }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(scratch);
    const size_t map_stride = (size_t)N * C * (H - 2 * SS_R) * (W - 2 * SS_R);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ssim_struct_fwd, dim3((unsigned)blocks), dim3(64), 0, st, target, pred, H, W, strips, chunks, win, wsum * wsum, partial,
                       maps, map_stride);
    const double inv = 1.0 / ((double)C * (H - 2 * SS_R) * (W - 2 * SS_R));
    hipLaunchKernelGGL(k_ssim_struct_fold, dim3((unsigned)N), dim3(64), 0, st, partial, C * strips * chunks, inv, structure);
    return gsr::launch_status();
}

__attribute__((visibility("default"))) int gsr_ssim_structure_bwd(const float *target, const float *pred, const float *maps,
                                                                  const float *grad_structure, int64_t N, int C, int H, int W,
                                                                  const float *window, float *grad_pred, void *stream)
{
    int strips, chunks;
    long long blocks;
    if (!target || !pred || !maps || !grad_structure || !window || !grad_pred || !ssim_grid(N, C, H, W, true, strips, chunks, blocks))
        return GSR_EINVAL;
    Window win;
    for (int q = 0; q < SS_WIN; ++q) win.w[q] = window[q];
    const size_t map_stride = (size_t)N * C * (H - 2 * SS_R) * (W - 2 * SS_R);
    const float inv_norm = (float)(1.0 / ((double)C * (H - 2 * SS_R) * (W - 2 * SS_R)));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ssim_struct_bwd, dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(stream), target, pred, maps, map_stride,
                       grad_structure, inv_norm, C, H, W, strips, chunks, win, grad_pred);
    return gsr::launch_status();
}

}  // extern "C"
