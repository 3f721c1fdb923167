// gsr_outputs.hip -- what a user takes away from a stylized scene: the cameras of the fly-through video, the video as bytes and the
// vertex table of the .ply export (src/visualization/camera_trajectory/, src/misc/utils.py::vis_depth_map, src/visualization/layout.py,
// src/model/ply_export.py), all on device memory.
//
//   gsr_trajectory     : interpolate_extrinsics / interpolate_intrinsics / the wobble transform, one thread per (pair, frame), float64
//                        inside and one rounding to float32 -- no Euler round trip through the host.
//   gsr_depth_range    : the log of the 99 % quantile of all depths and of the 1 % quantile of the positive ones, by the exact radix
//                        selection of gsr_select.h (no sort).
//   gsr_pack_frames    : clip / scale / cast / colour map / stack / flip / concatenate in ONE streaming pass: up to four planar fp32
//                        panels in, pixel-interleaved uint8 frames out, every lane 4 pixels = 3 full dwords.
//   gsr_ply_normalizer : (median xyz, factor) of export_ply(shift_and_scale=True), two selections.
//   gsr_ply_rows       : the packed fp32 vertex table; the quaternion goes through scipy's quat -> matrix -> quat round trip in float64.
//
// Selection: the engine is gsr_select.h.  This file supplies the source OSel -- a depth, a coordinate or |coordinate - median| as the
// value, the plan of each use (depth range: q 0.99 of all depths and q 0.01 of the positive ones; normaliser: the lower median, then
// q 0.95, per axis), no finish hook -- the chunk rule osel_chunks and the one-thread k_*_finish kernels that turn the selected values
// into the outputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"
#include "gsr_select.h"
#include "gsr_turbo_lut.h"

namespace gsr {

// bytes and selected values are compared bit for bit with the torch expression: fp32 products and sums stay separate
#pragma clang fp contract(off)

constexpr int OUT_BLOCK = 256, OSEL_MAX_MAPS = 3, OSEL_MAX_CHUNKS = 1024;
enum { OSEL_DEPTH = 0, OSEL_AXIS = 1, OSEL_ABSDEV = 2 };

struct OSelScratch {
    SelScratch sel;      // OSEL_MAX_MAPS maps
    float *aux;          // [OSEL_MAX_MAPS]: the medians the second selection of the normaliser subtracts
    size_t total;
};

static OSelScratch osel_carve(void *base)
{
    OSelScratch s;
    Carver c{base, 0};
    s.sel = sel_carve(c, OSEL_MAX_MAPS);
    s.aux = c.take<float>(OSEL_MAX_MAPS);
    s.total = c.off;
    return s;
}

struct OSel {
    const float *x;      // DEPTH: [n]; AXIS / ABSDEV: [n][3], map m reads column m
    const float *aux;    // ABSDEV: [3] medians
    long long n;
    int mode;
    float q0, q1;        // pair 0 over all elements, pair 1 over the positive ones (SEL_MEDIAN / SEL_UNUSED: gsr_select.h)
    __device__ SelPlan plan() const { return {{q0, q1}, {SEL_ALL, SEL_POSITIVE}}; }      // (subsets as constants: the kernels fold them)
    __device__ float value(int m, long long i, int) const
    {
        if (mode == OSEL_DEPTH) return x[i];
        const float v = x[3 * i + m];
        return mode == OSEL_AXIS ? v : fabsf(v - aux[m]);
    }
    __device__ void finish(int, const float *, const float *, bool) const {}      // (the k_*_finish kernels below read the scratch)
};

static int osel_chunks(long long n)
{
    long long c = (n + 4095) / 4096;
    return (int)(c < 1 ? 1 : (c > OSEL_MAX_CHUNKS ? OSEL_MAX_CHUNKS : c));
}

// ---- depth range ----
__device__ inline float log_once(float v) { return (float)log((double)v); }     // float64 inside: the correctly rounded fp32 logarithm

__global__ void k_depth_range_finish(const uint32_t *__restrict__ nanflag, const uint32_t *__restrict__ cnt, const float *__restrict__ w,
                                     const float *__restrict__ vals, float *__restrict__ range, int32_t *__restrict__ status)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float nanv = __uint_as_float(0x7fc00000u);
    const float q99 = nanflag[0] ? nanv : sel_lerp(vals[0], vals[1], w[0]);
    const uint32_t npos = cnt[1];
    const float q01 = npos ? sel_lerp(vals[2], vals[3], w[1]) : 0.f;
    range[0] = npos ? log_once(q01) : 0.f;       // (no positive depth: the reference's except branch)
    range[1] = log_once(q99);
    range[2] = q01;
    range[3] = q99;
    status[0] = (int32_t)npos;
    status[1] = npos ? 0 : GSR_DEPTH_NO_POSITIVE;
}

// ---- PLY normaliser ----
__global__ void k_ply_median_finish(const uint32_t *__restrict__ nanflag, const float *__restrict__ vals, float *__restrict__ aux, float *__restrict__ out)
{
    const int m = threadIdx.x;
    if (blockIdx.x != 0 || m >= 3) return;
    const float v = nanflag[m] ? __uint_as_float(0x7fc00000u) : vals[SEL_RANKS * m];
    aux[m] = v;
    out[m] = v;
}

__global__ void k_ply_factor_finish(const uint32_t *__restrict__ nanflag, const float *__restrict__ w, const float *__restrict__ vals, float *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float best = 0.f;
    bool nan = false;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const float q = sel_lerp(vals[SEL_RANKS * m], vals[SEL_RANKS * m + 1], w[2 * m]);
        nan |= nanflag[m] != 0u || q != q;
        best = (m == 0 || q > best) ? q : best;
    }
    out[3] = nan ? __uint_as_float(0x7fc00000u) : best;
}

// ---- PLY rows ----
struct PlyArgs {
    const float *means, *scales, *rot, *sh, *opac, *norm;
    long long G;
    int d_sh, n_rest, n_attr;
};

// R.from_quat(xyzw).as_matrix() -> R.from_matrix(...).as_quat(), component `which` of (w, x, y, z)
__device__ inline float ply_quat(const float *__restrict__ q, int which)
{
    double x = q[0], y = q[1], z = q[2], w = q[3];
    const double n = sqrt(x * x + y * y + z * z + w * w);
    if (!(n > 0.)) return which == 0 ? 1.f : 0.f;
    x /= n; y /= n; z /= n; w /= n;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w, xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    const double m00 = x2 - y2 - z2 + w2, m10 = 2. * (xy + zw), m20 = 2. * (xz - yw);
    const double m01 = 2. * (xy - zw), m11 = -x2 + y2 - z2 + w2, m21 = 2. * (yz + xw);
    const double m02 = 2. * (xz + yw), m12 = 2. * (yz - xw), m22 = -x2 - y2 + z2 + w2;
    const double tr = m00 + m11 + m22;
    int choice = 0;
    double best = m00;
    if (m11 > best) { best = m11; choice = 1; }
    if (m22 > best) { best = m22; choice = 2; }
    if (tr > best) { best = tr; choice = 3; }
    double ox, oy, oz, ow;
    if (choice == 0) { ox = 1. - tr + 2. * m00; oy = m10 + m01; oz = m20 + m02; ow = m21 - m12; }
    else if (choice == 1) { oy = 1. - tr + 2. * m11; oz = m21 + m12; ox = m01 + m10; ow = m02 - m20; }
    else if (choice == 2) { oz = 1. - tr + 2. * m22; ox = m02 + m20; oy = m12 + m21; ow = m10 - m01; }
    else { ox = m21 - m12; oy = m02 - m20; oz = m10 - m01; ow = 1. + tr; }
    const double on = sqrt(ox * ox + oy * oy + oz * oz + ow * ow);
    const double r = which == 0 ? ow : (which == 1 ? ox : (which == 2 ? oy : oz));
    return (float)(r / on);
}

// one thread per table element: the stores of a wavefront are 256 contiguous bytes whatever the row length is
__global__ void __launch_bounds__(OUT_BLOCK) k_ply_rows(PlyArgs a, float *__restrict__ rows)
{
    const long long total = a.G * a.n_attr;
    for (long long t = (long long)blockIdx.x * OUT_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * OUT_BLOCK) {
        const long long g = t / a.n_attr;
        int c = (int)(t - g * a.n_attr);
        float v;
        if (c < 3) {
            v = a.means[3 * g + c];
            if (a.norm) v = (v - a.norm[c]) / a.norm[3];
        } else if (c < 6) {
            v = 0.f;
        } else if (c < 9) {
            v = a.sh[(g * 3 + (c - 6)) * a.d_sh];
        } else if ((c -= 9) < a.n_rest) {
            const int ch = c / (a.d_sh - 1), k = c - ch * (a.d_sh - 1) + 1;
            v = a.sh[(g * 3 + ch) * a.d_sh + k];
        } else if ((c -= a.n_rest) == 0) {
            v = a.opac[g];
        } else if (c < 4) {
            float s = a.scales[3 * g + c - 1];
            if (a.norm) s = s / a.norm[3];
            v = log_once(s);
        } else {
            v = ply_quat(a.rot + 4 * g, c - 4);
        }
        rows[t] = v;
    }
}

// ---- trajectory ----
struct V3 { double x, y, z; };
__device__ inline V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ inline V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline V3 operator*(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// columns c0, c1, c2
struct M3 { V3 c0, c1, c2; };
__device__ inline V3 mul(const M3 &m, V3 v) { return m.c0 * v.x + m.c1 * v.y + m.c2 * v.z; }
__device__ inline V3 tmul(const M3 &m, V3 v) { return v3(dot(m.c0, v), dot(m.c1, v), dot(m.c2, v)); }      // m^T v
__device__ inline bool parallel(V3 a, V3 b, double eps) { return fabs(fabs(dot(a, b)) - 1.) < eps; }

struct Pose { M3 R; V3 o; };
__device__ inline Pose load_pose(const float *__restrict__ p)
{
    Pose r;
    r.R.c0 = v3(p[0], p[4], p[8]); r.R.c1 = v3(p[1], p[5], p[9]); r.R.c2 = v3(p[2], p[6], p[10]);
    r.o = v3(p[3], p[7], p[11]);
    return r;
}

// (n n^T - I) v
__device__ inline V3 nnt_minus_i(V3 n, V3 v) { return n * dot(n, v) - v; }

// least-squares intersection of the rays (oa, a), (ob, b): sum (n n^T - I) p = sum (n n^T - I) o, by the adjugate of the symmetric 3 x 3
__device__ inline V3 intersect_rays(V3 oa, V3 a, V3 ob, V3 b)
{
    const double m00 = a.x * a.x + b.x * b.x - 2., m11 = a.y * a.y + b.y * b.y - 2., m22 = a.z * a.z + b.z * b.z - 2.;
    const double m01 = a.x * a.y + b.x * b.y, m02 = a.x * a.z + b.x * b.z, m12 = a.y * a.z + b.y * b.z;
    const V3 r = nnt_minus_i(a, oa) + nnt_minus_i(b, ob);
    const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
    const double det = m00 * c00 + m01 * c01 + m02 * c02;
    return v3((c00 * r.x + c01 * r.y + c02 * r.z) / det, (c01 * r.x + c11 * r.y + c12 * r.z) / det, (c02 * r.x + c12 * r.y + c22 * r.z) / det);
}

// the 5 pivot parameters of a pose: translation in [axis x look, axis, look], then the Y and Z angles of the intrinsic "YXZ" Euler
// decomposition of frame^T R = Ry Rx Rz (the X angle is dropped)
__device__ inline void pivot_params(const Pose &e, const M3 &frame, V3 pivot, V3 &tr, double &ay, double &az)
{
    M3 tf;
    tf.c0 = cross(frame.c1, e.R.c2); tf.c1 = frame.c1; tf.c2 = e.R.c2;
    tr = tmul(tf, pivot - e.o);
    // M = frame^T R, by columns
    const V3 q0 = tmul(frame, e.R.c0), q1 = tmul(frame, e.R.c1), q2 = tmul(frame, e.R.c2);
    const double m10 = q0.y, m11 = q1.y;                 // cos X sin Z, cos X cos Z
    const double m02 = q2.x, m22 = q2.z;                 // sin Y cos X, cos Y cos X
    if (m10 * m10 + m11 * m11 < 1e-24) {                 // gimbal lock (|cos X| below float64 noise): scipy's rule, third angle 0
        az = 0.;
        ay = q2.y < 0. ? atan2(q1.x, q0.x) : atan2(-q1.x, q0.x);          // sin X = -m12: +1 -> (m01, m00) = (sin, cos)(Y - Z)
    } else {
        ay = atan2(m02, m22);
        az = atan2(m10, m11);
    }
}

__device__ inline double mod_tau(double a, double tau)
{
    double r = fmod(a, tau);
    if (r != 0. && r < 0.) r += tau;
    return r;
}
// interpolate_circular: mod 2 pi, the shorter way round, with the reference's tie rules
__device__ inline double lerp_circular(double a, double b, double t)
{
    const double tau = 2. * 3.141592653589793;
    a = mod_tau(a, tau);
    b = mod_tau(b, tau);
    const double d = fabs(b - a), al = a - tau, dl = fabs(b - al), ar = a + tau, dr = fabs(b - ar);
    const bool use_d = d < dl && d < dr, use_l = dl < dr && !use_d;
    const double a0 = use_d ? a : (use_l ? al : ar);
    return a0 + (b - a0) * t;
}

struct TrajArgs {
    const float *a, *b, *Ka, *Kb, *t, *radius;
    int P, F;
    float t_scale, t_shift, eps;
    int hold_a;
    float wob_factor;
    int wob_rotations, wob_scale_t;
};

__global__ void __launch_bounds__(64) k_trajectory(TrajArgs g, float *__restrict__ c2w, float *__restrict__ K)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= g.P * g.F) return;
    const int p = idx / g.F, f = idx - p * g.F;
    const float t32 = g.t[f];
    const float tm32 = t32 * g.t_scale + g.t_shift;         // (fp32, two roundings: the caller's `t * 5 - 2` on a float32 tensor)
    const double tm = tm32;
    const Pose A = load_pose(g.a + 16 * p), B = load_pose(g.b + 16 * p);
    float *out = c2w + 16 * (size_t)idx, *ko = K + 9 * (size_t)idx;
    const float *ka = g.Ka + 9 * p, *kb = g.Kb + 9 * p;
#pragma unroll
    for (int j = 0; j < 9; ++j) ko[j] = g.hold_a ? ka[j] : ka[j] + (kb[j] - ka[j]) * tm32;
    Pose E;
    if (g.hold_a) {
        E = A;
    } else {
        const double eps = g.eps;
        const V3 a = A.R.c2, b = B.R.c2;
        V3 pivot = (A.o + B.o) * 0.5;
        if (!parallel(a, b, eps)) pivot = intersect_rays(A.o, a, B.o, b);
        V3 b2 = b;
        if (parallel(a, b2, eps)) b2 = v3(0., 0., 1.);
        if (parallel(a, b2, eps)) b2 = v3(0., 1., 0.);
        V3 y = cross(a, b2);
        y = y * (1. / sqrt(dot(y, y)));
        M3 frame;
        frame.c0 = cross(y, a); frame.c1 = y; frame.c2 = a;
        V3 ta, tb;
        double ya, za, yb, zb;
        pivot_params(A, frame, pivot, ta, ya, za);
        pivot_params(B, frame, pivot, tb, yb, zb);
        const V3 tr = ta + (tb - ta) * tm;
        const double ay = lerp_circular(ya, yb, tm), az = lerp_circular(za, zb, tm);
        // Ry(ay) Rz(az), by columns
        const double cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
        E.R.c0 = mul(frame, v3(cy * cz, sz, -sy * cz));
        E.R.c1 = mul(frame, v3(-cy * sz, cz, sy * sz));
        E.R.c2 = mul(frame, v3(sy, 0., cy));
        M3 tf;
        tf.c0 = cross(y, E.R.c2); tf.c1 = y; tf.c2 = E.R.c2;
        E.o = pivot - mul(tf, tr);
    }
    if (g.wob_factor != 0.f) {
        // right-multiplied translation in the image plane, on the UNMAPPED t
        const double t = t32;
        const V3 dd = A.o - B.o;
        double r = (double)g.wob_factor * (g.radius ? (double)g.radius[p] : sqrt(dot(dd, dd)));
        if (g.wob_scale_t) r *= t;
        const double ang = 2. * 3.141592653589793 * (double)g.wob_rotations * t;
        E.o = E.o + E.R.c0 * (sin(ang) * r) + E.R.c1 * (-cos(ang) * r);
    }
    const bool exact = g.hold_a && g.wob_factor == 0.f;
    if (exact) {
        const float *src = g.a + 16 * p;
#pragma unroll
        for (int j = 0; j < 16; ++j) out[j] = src[j];
        return;
    }
    out[0] = (float)E.R.c0.x; out[1] = (float)E.R.c1.x; out[2] = (float)E.R.c2.x; out[3] = (float)E.o.x;
    out[4] = (float)E.R.c0.y; out[5] = (float)E.R.c1.y; out[6] = (float)E.R.c2.y; out[7] = (float)E.o.y;
    out[8] = (float)E.R.c0.z; out[9] = (float)E.R.c1.z; out[10] = (float)E.R.c2.z; out[11] = (float)E.o.z;
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
}

// ---- frames ----
struct PackArgs {
    const float *p0, *p1, *p2, *p3;
    int depth_mask;            // bit i: panel i is a depth (F,H,W), otherwise planar RGB (F,3,H,W)
    int n_panels, F, H, W, axis, gap, Fo, Ho, Wo;
    const float *range;        // near, far (logs)
    uint8_t *out;
    long long total_px;
};

__device__ inline uint32_t byte_of(float x)
{
    if (x != x) return 0u;
    return (uint32_t)(int)(fminf(fmaxf(x, 0.f), 1.f) * 255.0f);
}
__device__ inline uint32_t turbo_of(float d, float near, float far, const uint32_t *lut)
{
    const float x = 1.0f - (log_once(d) - near) / (far - near);      // (the correctly rounded log: the bytes do not depend on a libm)
    if (x != x) return 0u;                                               // matplotlib's "bad" colour
    const int i = (int)(fminf(fmaxf(x, 0.f), 1.f) * 256.0f);
    return lut[i > 255 ? 255 : i];
}

struct PxSrc { const float *base; int depth; long long off; bool gap; };   // off: index of the pixel in plane 0 of its frame

__device__ inline PxSrc px_locate(const PackArgs &a, long long pix)
{
    const long long frame_px = (long long)a.Ho * a.Wo;
    const int fo = (int)(pix / frame_px), rem = (int)(pix - fo * frame_px);
    const int y = rem / a.Wo, x = rem - y * a.Wo;
    const int f = fo < a.F ? fo : 2 * a.F - 2 - fo;
    const int main = a.axis == 0 ? y : x, span = a.axis == 0 ? a.H : a.W;
    const int pi = main / (span + a.gap), o = main - pi * (span + a.gap);
    PxSrc s;
    s.gap = o >= span;
    s.depth = (a.depth_mask >> pi) & 1;
    s.base = pi == 0 ? a.p0 : (pi == 1 ? a.p1 : (pi == 2 ? a.p2 : a.p3));
    const int ys = a.axis == 0 ? o : y, xs = a.axis == 0 ? x : o;
    s.off = (long long)f * (s.depth ? 1 : 3) * a.H * a.W + (long long)ys * a.W + xs;
    return s;
}

__device__ inline uint32_t px_colour(const PackArgs &a, const PxSrc &s, float near, float far, const uint32_t *lut)
{
    if (s.gap) return 0xffffffu;
    if (s.depth) return turbo_of(s.base[s.off], near, far, lut);
    const long long hw = (long long)a.H * a.W;
    return byte_of(s.base[s.off]) | (byte_of(s.base[s.off + hw]) << 8) | (byte_of(s.base[s.off + 2 * hw]) << 16);
}

// a lane owns output pixels 4 i .. 4 i + 3 of the flat (F', H_out, W_out) stream: 12 bytes, three aligned dwords
__global__ void __launch_bounds__(OUT_BLOCK) k_pack_frames(PackArgs a)
{
    __shared__ uint32_t lut[256];
    lut[threadIdx.x] = TURBO_LUT[threadIdx.x];
    __syncthreads();
    const long long lane = (long long)blockIdx.x * OUT_BLOCK + threadIdx.x, pix = 4 * lane;
    if (pix >= a.total_px) return;
    float near = 0.f, far = 0.f;
    if (a.depth_mask) { near = a.range[0]; far = a.range[1]; }
    uint32_t c[4];
    const PxSrc s0 = px_locate(a, pix);
    const long long frame_px = (long long)a.Ho * a.Wo;
    const int x0 = (int)((pix % frame_px) % a.Wo);
    bool quad = pix + 3 < a.total_px && x0 + 3 < a.Wo && !s0.gap;
    if (quad && a.axis == 1) {                               // the four pixels in one panel?
        const int o = x0 % (a.W + a.gap);
        quad = o + 3 < a.W;
    }
    quad = quad && ((reinterpret_cast<uintptr_t>(s0.base + s0.off) & 15u) == 0u) && (((long long)a.H * a.W) & 3) == 0;
    if (quad) {
        if (s0.depth) {
            const float4 d = *reinterpret_cast<const float4 *>(s0.base + s0.off);
            c[0] = turbo_of(d.x, near, far, lut); c[1] = turbo_of(d.y, near, far, lut);
            c[2] = turbo_of(d.z, near, far, lut); c[3] = turbo_of(d.w, near, far, lut);
        } else {
            const long long hw = (long long)a.H * a.W;
            const float4 r = *reinterpret_cast<const float4 *>(s0.base + s0.off);
            const float4 g = *reinterpret_cast<const float4 *>(s0.base + s0.off + hw);
            const float4 b = *reinterpret_cast<const float4 *>(s0.base + s0.off + 2 * hw);
            c[0] = byte_of(r.x) | (byte_of(g.x) << 8) | (byte_of(b.x) << 16);
            c[1] = byte_of(r.y) | (byte_of(g.y) << 8) | (byte_of(b.y) << 16);
            c[2] = byte_of(r.z) | (byte_of(g.z) << 8) | (byte_of(b.z) << 16);
            c[3] = byte_of(r.w) | (byte_of(g.w) << 8) | (byte_of(b.w) << 16);
        }
    } else {
        c[0] = px_colour(a, s0, near, far, lut);
#pragma unroll
        for (int j = 1; j < 4; ++j) c[j] = pix + j < a.total_px ? px_colour(a, px_locate(a, pix + j), near, far, lut) : 0u;
    }
    if (pix + 3 < a.total_px) {
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + 3 * pix);
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
    } else {                                                 // the stream's last 1 - 3 pixels: bytes
        const int left = (int)(a.total_px - pix);
        uint8_t *o = a.out + 3 * pix;
        if (left > 0) { o[0] = (uint8_t)c[0]; o[1] = (uint8_t)(c[0] >> 8); o[2] = (uint8_t)(c[0] >> 16); }
        if (left > 1) { o[3] = (uint8_t)c[1]; o[4] = (uint8_t)(c[1] >> 8); o[5] = (uint8_t)(c[1] >> 16); }
        if (left > 2) { o[6] = (uint8_t)c[2]; o[7] = (uint8_t)(c[2] >> 8); o[8] = (uint8_t)(c[2] >> 16); }
    }
}

#pragma clang fp contract(fast)

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) int gsr_trajectory(const float *c2w_a, const float *c2w_b, const float *K_a, const float *K_b,
                                                          const float *t, int P, int F, float t_scale, float t_shift, float eps, int hold_a,
                                                          float wobble_factor, int wobble_rotations, int wobble_scale_with_t,
                                                          const float *wobble_radius, float *c2w, float *K, void *stream)
{
    using namespace gsr;
    if (!c2w_a || !c2w_b || !K_a || !K_b || !t || !c2w || !K || P < 1 || F < 1 || (long long)P * F > (1LL << 24)) return GSR_EINVAL;
    if (!(eps > 0.f) || !(t_scale == t_scale) || !(t_shift == t_shift) || !(wobble_factor == wobble_factor)) return GSR_EINVAL;
    TrajArgs g{c2w_a, c2w_b, K_a, K_b, t, wobble_radius, P, F, t_scale, t_shift, eps, hold_a ? 1 : 0, wobble_factor, wobble_rotations,
               wobble_scale_with_t ? 1 : 0};
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_trajectory, dim3((unsigned)((P * F + 63) / 64)), dim3(64), 0, static_cast<hipStream_t>(stream), g, c2w, K);
    return launch_status();
}

__attribute__((visibility("default"))) size_t gsr_outputs_scratch_bytes(void) { return gsr::osel_carve(nullptr).total; }

__attribute__((visibility("default"))) int gsr_depth_range(const float *depth, int64_t n, int64_t max_elems, void *scratch, float *range,
                                                           int32_t *status, void *stream)
{
    using namespace gsr;
    if (!depth || !scratch || !range || !status || n < 1 || max_elems < 1) return GSR_EINVAL;
    const long long ne = n < max_elems ? n : max_elems;
    if (ne > (1LL << 31)) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const OSelScratch sc = osel_carve(scratch);
    const SelScratch &ss = sc.sel;
    if (!hip_ok(hipMemsetAsync(ss.hist, 0, sel_zero_bytes(ss), s))) return GSR_ELAUNCH;
    (void)hipGetLastError();
    sel_run(OSel{depth, nullptr, ne, OSEL_DEPTH, 0.99f, 0.01f}, 1, osel_chunks(ne), ss, s);
    hipLaunchKernelGGL(k_depth_range_finish, dim3(1), dim3(64), 0, s, ss.nanflag, ss.cnt, ss.w, ss.vals, range, status);
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_pack_frames(const float *const *panels, const int32_t *is_depth, int n_panels, int F, int H,
                                                           int W, int axis, int gap, int loop_reverse, const float *range, uint8_t *out,
                                                           void *stream)
{
    using namespace gsr;
    if (!panels || !is_depth || !out || n_panels < 1 || n_panels > 4 || F < 1 || H < 1 || W < 1 || axis < 0 || axis > 1 || gap < 0) return GSR_EINVAL;
    PackArgs a{};
    const float *p[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < n_panels; ++i) {
        if (!panels[i]) return GSR_EINVAL;
        p[i] = panels[i];
        if (is_depth[i]) a.depth_mask |= 1 << i;
    }
    if (a.depth_mask && !range) return GSR_EINVAL;
    a.p0 = p[0]; a.p1 = p[1]; a.p2 = p[2]; a.p3 = p[3];
    a.n_panels = n_panels; a.F = F; a.H = H; a.W = W; a.axis = axis; a.gap = gap;
    a.Fo = loop_reverse ? F + (F > 2 ? F - 2 : 0) : F;
    const long long ho = axis == 0 ? (long long)n_panels * H + (long long)(n_panels - 1) * gap : H;
    const long long wo = axis == 1 ? (long long)n_panels * W + (long long)(n_panels - 1) * gap : W;
    if (ho * wo >= (1LL << 31) || (long long)F * 3 * H * W >= (1LL << 40)) return GSR_EINVAL;
    a.Ho = (int)ho; a.Wo = (int)wo;
    a.range = range; a.out = out;
    a.total_px = (long long)a.Fo * ho * wo;
    const long long lanes = (a.total_px + 3) / 4, groups = (lanes + OUT_BLOCK - 1) / OUT_BLOCK;
    if (groups >= (1LL << 31)) return GSR_EINVAL;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pack_frames, dim3((unsigned)groups), dim3(OUT_BLOCK), 0, static_cast<hipStream_t>(stream), a);
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_ply_normalizer(const float *means, int64_t G, void *scratch, float *out, void *stream)
{
    using namespace gsr;
    if (!means || !scratch || !out || G < 2 || G > (1LL << 31)) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const OSelScratch sc = osel_carve(scratch);
    const SelScratch &ss = sc.sel;
    const int chunks = osel_chunks(G);
    if (!hip_ok(hipMemsetAsync(ss.hist, 0, sel_zero_bytes(ss), s))) return GSR_ELAUNCH;
    (void)hipGetLastError();
    sel_run(OSel{means, nullptr, (long long)G, OSEL_AXIS, SEL_MEDIAN, SEL_UNUSED}, 3, chunks, ss, s);
    hipLaunchKernelGGL(k_ply_median_finish, dim3(1), dim3(64), 0, s, ss.nanflag, ss.vals, sc.aux, out);
    // (the picks left the histograms at zero; a NaN flag stays up: |x - median| of that axis holds the NaN again)
    sel_run(OSel{means, sc.aux, (long long)G, OSEL_ABSDEV, 0.95f, SEL_UNUSED}, 3, chunks, ss, s);
    hipLaunchKernelGGL(k_ply_factor_finish, dim3(1), dim3(64), 0, s, ss.nanflag, ss.w, ss.vals, out);
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_ply_rows(const float *means, const float *scales, const float *rotations, const float *harmonics,
                                                        const float *opacities, int64_t G, int d_sh, int dc_only, const float *normalizer,
                                                        float *rows, void *stream)
{
    using namespace gsr;
    if (!means || !scales || !rotations || !harmonics || !opacities || !rows || G < 1 || G > (1LL << 31) || d_sh < 1 || d_sh > 64) return GSR_EINVAL;
    PlyArgs a{means, scales, rotations, harmonics, opacities, normalizer, (long long)G, d_sh, dc_only ? 0 : 3 * (d_sh - 1), 0};
    a.n_attr = 17 + a.n_rest;
    long long groups = (a.G * a.n_attr + OUT_BLOCK - 1) / OUT_BLOCK;
    if (groups > 16384) groups = 16384;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ply_rows, dim3((unsigned)groups), dim3(OUT_BLOCK), 0, static_cast<hipStream_t>(stream), a, rows);
    return launch_status();
}

}  // extern "C"
