// gsr_views.hip -- view selection: the mutual overlap of two views, the number the reference's evaluation-index generator steers by
// (src/evaluation/evaluation_index_generator.py through src/geometry/epipolar_lines.py::project_rays with near = far = None).  For a
// pair (a, b) every pixel of a sends its ray into b; the ray counts when the projection of its segment [0, inf) crosses b's image.
// The reference evaluates one pair at a time in about two hundred small tensor ops and reads two means back per pair; here every
// candidate pair of a context frame, both directions, is ONE launch and one int32 count per (pair, direction).
//
//   k_view_tables  : one thread per view widens its fp32 cameras and forms both inverses in float64 -- the 3 x 3 by the adjugate, the
//                    4 x 4 by complementary 2 x 2 minors (general, not a rigid transpose).  The same launch re-arms the counters: 0,
//                    or -1 for a pair that names a view outside [0, V).
//   k_view_overlap : grid (2 P directions, ray blocks).  A lane generates its ray from the pixel index -- (idx + 0.5) / length in
//                    fp32 as the reference's sample_image_grid forms it, then widened -- and restates get_world_rays and
//                    project_rays in float64.  Only the boolean leaves the lane: 64-bit ballot, popcount, one integer add per
//                    block.  Integer adds commute: two runs give the same counts.  No float atomics.
//
// Every rule of the reference is kept: division by z + 2^-23 and nan_to_num(NaN -> 0, +-inf -> +-1e8) in the camera projection, the
// 1e-6 of the three predicates, the four unprotected frame intersections (inf / NaN flow through IEEE comparisons), the min / max
// SELECTION among the four (invalid entries overwritten by +-inf, first index wins a tie, the selected entry's own flag is
// returned -- not "any is valid"), the at-camera / zero-depth rules and the final (zero | frame-min) x (infinity | frame-max) choice.
//
// Floating-point contraction is off in this file: each product and sum rounds once, in the order written, which is the order of the
// host restatement in styl3r_amd/views.py.  No fast-math.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"

#pragma clang fp contract(off)

namespace gsr {

constexpr int VW_BLOCK = 256;
constexpr int VW_K = 0, VW_KINV = 9, VW_E = 18, VW_EINV = 34, VW_C = 50, VW_DOUBLES = 54;       // one view's table
constexpr double VW_EPS = 1e-6, VW_ONE_EPS = 1 + 1e-6, VW_Z_EPS = 1.1920928955078125e-07, VW_BIG = 1e8;

__global__ void __launch_bounds__(VW_BLOCK) k_view_tables(const float *__restrict__ extrinsics, const float *__restrict__ intrinsics, int V,
                                                           const int32_t *__restrict__ pairs, long long P, double *__restrict__ tables,
                                                           int32_t *__restrict__ counts)
{
    const long long i = (long long)blockIdx.x * VW_BLOCK + threadIdx.x;
    if (i < P) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        const int32_t arm = (a >= 0 && a < V && b >= 0 && b < V) ? 0 : -1;
        counts[2 * i] = arm;
        counts[2 * i + 1] = arm;
    }
    if (i >= V) return;
    double *t = tables + (size_t)i * VW_DOUBLES;
    double k[9], m[16];
    for (int q = 0; q < 9; ++q) k[q] = (double)intrinsics[i * 9 + q];
    for (int q = 0; q < 16; ++q) m[q] = (double)extrinsics[i * 16 + q];
    {   // 3 x 3: cofactors over the determinant
        const double c00 = k[4] * k[8] - k[5] * k[7], c01 = k[2] * k[7] - k[1] * k[8], c02 = k[1] * k[5] - k[2] * k[4];
        const double c10 = k[5] * k[6] - k[3] * k[8], c11 = k[0] * k[8] - k[2] * k[6], c12 = k[2] * k[3] - k[0] * k[5];
        const double c20 = k[3] * k[7] - k[4] * k[6], c21 = k[1] * k[6] - k[0] * k[7], c22 = k[0] * k[4] - k[1] * k[3];
        const double det = (k[0] * c00 + k[1] * c10) + k[2] * c20;
        const double inv[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};
        for (int q = 0; q < 9; ++q) {
            t[VW_K + q] = k[q];
            t[VW_KINV + q] = inv[q] / det;
        }
        // the frame lines x = 0, x = 1, y = 0, y = 1 as camera-space slopes (value - c) / f: the same for every ray into this view
        t[VW_C + 0] = (0.0 - k[2]) / k[0];
        t[VW_C + 1] = (1.0 - k[2]) / k[0];
        t[VW_C + 2] = (0.0 - k[5]) / k[4];
        t[VW_C + 3] = (1.0 - k[5]) / k[4];
    }
    {   // 4 x 4: 2 x 2 minors of the upper (s) and the lower (c) row pair
#define A(r, c) m[(r) * 4 + (c)]
        const double s0 = A(0, 0) * A(1, 1) - A(1, 0) * A(0, 1), s1 = A(0, 0) * A(1, 2) - A(1, 0) * A(0, 2), s2 = A(0, 0) * A(1, 3) - A(1, 0) * A(0, 3);
        const double s3 = A(0, 1) * A(1, 2) - A(1, 1) * A(0, 2), s4 = A(0, 1) * A(1, 3) - A(1, 1) * A(0, 3), s5 = A(0, 2) * A(1, 3) - A(1, 2) * A(0, 3);
        const double c5 = A(2, 2) * A(3, 3) - A(3, 2) * A(2, 3), c4 = A(2, 1) * A(3, 3) - A(3, 1) * A(2, 3), c3 = A(2, 1) * A(3, 2) - A(3, 1) * A(2, 2);
        const double c2 = A(2, 0) * A(3, 3) - A(3, 0) * A(2, 3), c1 = A(2, 0) * A(3, 2) - A(3, 0) * A(2, 2), c0 = A(2, 0) * A(3, 1) - A(3, 0) * A(2, 1);
        const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
        const double adj[16] = {
            (A(1, 1) * c5 - A(1, 2) * c4) + A(1, 3) * c3, (A(0, 2) * c4 - A(0, 1) * c5) - A(0, 3) * c3,
            (A(3, 1) * s5 - A(3, 2) * s4) + A(3, 3) * s3, (A(2, 2) * s4 - A(2, 1) * s5) - A(2, 3) * s3,
            (A(1, 2) * c2 - A(1, 0) * c5) - A(1, 3) * c1, (A(0, 0) * c5 - A(0, 2) * c2) + A(0, 3) * c1,
            (A(3, 2) * s2 - A(3, 0) * s5) - A(3, 3) * s1, (A(2, 0) * s5 - A(2, 2) * s2) + A(2, 3) * s1,
            (A(1, 0) * c4 - A(1, 1) * c2) + A(1, 3) * c0, (A(0, 1) * c2 - A(0, 0) * c4) - A(0, 3) * c0,
            (A(3, 0) * s4 - A(3, 1) * s2) + A(3, 3) * s0, (A(2, 1) * s2 - A(2, 0) * s4) - A(2, 3) * s0,
            (A(1, 1) * c1 - A(1, 0) * c3) - A(1, 2) * c0, (A(0, 0) * c3 - A(0, 1) * c1) + A(0, 2) * c0,
            (A(3, 1) * s1 - A(3, 0) * s3) - A(3, 2) * s0, (A(2, 0) * s3 - A(2, 1) * s1) + A(2, 2) * s0};
#undef A
        for (int q = 0; q < 16; ++q) {
            t[VW_E + q] = m[q];
            t[VW_EINV + q] = adj[q] / det;
        }
    }
}

__device__ __forceinline__ bool vw_in01(double v) { return (v >= -VW_EPS) & (v <= VW_ONE_EPS); }

__device__ __forceinline__ double vw_nan_to_num(double v)
{
    v = v != v ? 0.0 : v;
    v = v == INFINITY ? VW_BIG : v;
    return v == -INFINITY ? -VW_BIG : v;
}

// project_camera_space + _is_in_bounds + _is_in_front_of_camera of one camera-space point (t's own test is the caller's)
__device__ __forceinline__ bool vw_point_valid(const double *__restrict__ K, double px, double py, double pz)
{
    const double den = pz + VW_Z_EPS;
    const double qx = vw_nan_to_num(px / den), qy = vw_nan_to_num(py / den), qz = vw_nan_to_num(pz / den);
    const double x = (K[0] * qx + K[1] * qy) + K[2] * qz, y = (K[3] * qx + K[4] * qy) + K[5] * qz;
    return vw_in01(x) & vw_in01(y) & (pz > -VW_EPS);
}

// _intersect_image_coordinate: the ray's projection against the frame line {same = value}, c = (value - cs) / fs from the table
__device__ __forceinline__ bool vw_frame_hit(double fo, double co, double c, double os, double oo, double oz, double ds, double dn, double dz,
                                             double &t)
{
    t = (c * oz - os) / (ds - c * dz);
    const double other = co + (fo * (oo * (c * dz - ds) + dn * (os - c * oz))) / (dz * os - ds * oz);
    return vw_in01(other) & (oz + t * dz > -VW_EPS) & (t > -VW_EPS);
}

__global__ void __launch_bounds__(VW_BLOCK) k_view_overlap(const double *__restrict__ tables, const int32_t *__restrict__ pairs, int V, int H,
                                                            int W, int32_t *__restrict__ counts)
{
    __shared__ int s_count;
    const long long dir = blockIdx.x;                       // 2 p + (0: pairs[p][0] -> pairs[p][1], 1: the other way)
    const int a = pairs[dir], b = pairs[dir ^ 1];
    if (a < 0 || a >= V || b < 0 || b >= V) return;          // (block-uniform; the prologue wrote -1)
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const double *__restrict__ ta = tables + (size_t)a * VW_DOUBLES, *__restrict__ tb = tables + (size_t)b * VW_DOUBLES;
    const double *__restrict__ Ki = ta + VW_KINV, *__restrict__ E = ta + VW_E, *__restrict__ M = tb + VW_EINV, *__restrict__ K = tb + VW_K,
                 *__restrict__ Cf = tb + VW_C;
    // the origin of a's rays in b's camera space
    const double wx = E[3], wy = E[7], wz = E[11];
    const double ox = ((M[0] * wx + M[1] * wy) + M[2] * wz) + M[3];
    const double oy = ((M[4] * wx + M[5] * wy) + M[6] * wz) + M[7];
    const double oz = ((M[8] * wx + M[9] * wy) + M[10] * wz) + M[11];
    const bool at_camera = sqrt((ox * ox + oy * oy) + oz * oz) < VW_EPS, depth_zero = oz < VW_EPS;
    const int n_rays = H * W;
    const float fw = (float)W, fh = (float)H;
    int mine = 0;
    for (int base = blockIdx.y * VW_BLOCK; base < n_rays; base += gridDim.y * VW_BLOCK) {
        const int r = base + threadIdx.x;
        const bool live = r < n_rays;
        const int rr = live ? r : 0, row = rr / W, col = rr - row * W;
        const double x = (double)(((float)col + 0.5f) / fw), y = (double)(((float)row + 0.5f) / fh);
        // get_world_rays: unproject at depth one, normalise, rotate into the world
        double cx = (Ki[0] * x + Ki[1] * y) + Ki[2], cy = (Ki[3] * x + Ki[4] * y) + Ki[5], cz = (Ki[6] * x + Ki[7] * y) + Ki[8];
        const double len = sqrt((cx * cx + cy * cy) + cz * cz);
        cx = cx / len; cy = cy / len; cz = cz / len;
        const double ux = (E[0] * cx + E[1] * cy) + E[2] * cz, uy = (E[4] * cx + E[5] * cy) + E[6] * cz, uz = (E[8] * cx + E[9] * cy) + E[10] * cz;
        // project_rays: into b's camera space
        const double dx = (M[0] * ux + M[1] * uy) + M[2] * uz, dy = (M[4] * ux + M[5] * uy) + M[6] * uz, dz = (M[8] * ux + M[9] * uy) + M[10] * uz;
        double t[4];
        bool v[4];
        v[0] = vw_frame_hit(K[4], K[5], Cf[0], ox, oy, oz, dx, dy, dz, t[0]);
        v[1] = vw_frame_hit(K[4], K[5], Cf[1], ox, oy, oz, dx, dy, dz, t[1]);
        v[2] = vw_frame_hit(K[0], K[2], Cf[2], oy, ox, oz, dy, dx, dz, t[2]);
        v[3] = vw_frame_hit(K[0], K[2], Cf[3], oy, ox, oz, dy, dx, dz, t[3]);
        // _compare_projections: invalid entries lose, the first index wins a tie, the selected entry's flag is the answer
        double lo = v[0] ? t[0] : INFINITY, hi = v[0] ? t[0] : -INFINITY;
        bool lo_valid = v[0], hi_valid = v[0];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const double tl = v[q] ? t[q] : INFINITY, th = v[q] ? t[q] : -INFINITY;
            const bool less = tl < lo, more = th > hi;
            lo = less ? tl : lo; lo_valid = less ? v[q] : lo_valid;
            hi = more ? th : hi; hi_valid = more ? v[q] : hi_valid;
        }
        // zero depth: the origin, or the direction when the origin is the camera itself; an origin on the zero plane elsewhere is out
        const bool zero_valid = vw_point_valid(K, at_camera ? dx : ox, at_camera ? dy : oy, at_camera ? dz : oz) & !(depth_zero & !at_camera);
        const bool inf_valid = vw_point_valid(K, dx, dy, dz);
        const bool overlaps = (zero_valid | lo_valid) & (inf_valid | hi_valid) & live;
        mine += __popcll(__ballot(overlaps));                // (the same number in every lane of the wave)
    }
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(counts + dir, s_count);
}

static bool view_dims_ok(int V, int64_t P, int H, int W)
{
    return V >= 1 && P >= 1 && P <= (1LL << 22) && H >= 1 && W >= 1 && (int64_t)H * W <= (1LL << 24);
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_view_overlap_scratch_bytes(int V, int64_t P)
{
    if (V < 1 || P < 1 || P > (1LL << 22)) return 0;
    return (size_t)V * gsr::VW_DOUBLES * sizeof(double);
}

__attribute__((visibility("default"))) int gsr_view_overlap(const float *extrinsics, const float *intrinsics, int V, const int32_t *pairs, int64_t P,
                                                            int H, int W, void *scratch, size_t scratch_bytes, int32_t *counts, void *stream)
{
    using namespace gsr;
    if (!extrinsics || !intrinsics || !pairs || !scratch || !counts || !view_dims_ok(V, P, H, W)) return GSR_EINVAL;
    if (reinterpret_cast<uintptr_t>(scratch) & 7) return GSR_EINVAL;
    if (scratch_bytes < (size_t)V * VW_DOUBLES * sizeof(double)) return GSR_ENOSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *tables = static_cast<double *>(scratch);
    const long long n_pro = P > V ? (long long)P : V;
    const int ray_blocks = (H * W + VW_BLOCK - 1) / VW_BLOCK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_view_tables, dim3((unsigned)((n_pro + VW_BLOCK - 1) / VW_BLOCK)), dim3(VW_BLOCK), 0, s, extrinsics, intrinsics, V, pairs,
                       (long long)P, tables, counts);
    hipLaunchKernelGGL(k_view_overlap, dim3((unsigned)(2 * P), (unsigned)(ray_blocks < 65535 ? ray_blocks : 65535)), dim3(VW_BLOCK), 0, s, tables,
                       pairs, V, H, W, counts);
    return launch_status();
}

}  // extern "C"
