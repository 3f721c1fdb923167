// gsr_points.hip -- point-map distillation (src/model/distiller, src/loss/loss_point.py::Regr3D) on device memory.
//
//   gsr_pointmap_post : the teacher head's post-processing (heads/postprocess.py, depth mode ('exp', -inf, inf), conf mode ('exp', 1, inf))
//                       in one pass over the (P,4,H,W) head output.
//   gsr_regr3d_fwd    : Regr3D.  Per (view, image) map the 0.2 % / 99.8 % quantiles of |gt| by the exact radix selection of
//                       gsr_select.h -- the four ranks floor / ceil of both quantile positions followed together -- instead of
//                       torch.quantile's two full row sorts; then the valid mask, the joint avg_dis normalisation and the masked
//                       Euclidean distance, reduced through per-workgroup float64 partials that ONE thread per map folds in index
//                       order (two runs are bit-identical).
//   gsr_regr3d_bwd    : one element-wise pass; the per-image reduction the avg_dis scale needs is left behind by the forward.
//
// Selection: the engine (keys, histogram and pick kernels, ranks, scratch, launch loop) is gsr_select.h.  This file supplies the source
// PtSel -- |gt| computed and stored to `dis` on pass 0 and read back afterwards, both quantiles over all points, the lerp with the NaN
// override as the finish -- the chunk rule pt_chunks, and k_sel_one: maps of at most SEL_ONE_MAX_N points take ONE workgroup each
// (keys in registers, histogram and pick in LDS, one launch instead of eight), built from the engine's key, bump, pick and ranks and
// from PtSel's value and finish.  Nothing syncs with the host, there are no float atomics, and the launch sequence depends on
// (B, N, mode) only.
//
// Deviation from the reference (deliberate): a view whose valid set is empty contributes 0 with a zero gradient (the reference
// returns NaN, the mean of an empty tensor); `status` reports it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr.h"
#include "gsr_common.h"
#include "gsr_select.h"

namespace gsr {

// |gt| decides mask membership against quantiles that are themselves values of |gt|: every kernel must see the same bits
#pragma clang fp contract(off)

constexpr int PT_BLOCK = 256, PT_MAX_CHUNKS = 64;
constexpr int SEL_ONE_BLOCK = 1024, SEL_ONE_KEYS = 8;
constexpr long long SEL_ONE_MAX_N = (long long)SEL_ONE_BLOCK * SEL_ONE_KEYS;
constexpr float CONF_MIN = 3.0f;

struct PtScratch {
    float *dis;          // [2B][N]   |gt|
    uint8_t *mask;       // [2B][N]   valid
    SelScratch sel;      // [2B] maps
    float *quant;        // [2B][2]
    double *part;        // [2B][PT_MAX_CHUNKS][4]: count, sum |pr|, sum |gt|, sum |pr - gt|
    double *part2;       // [2B][PT_MAX_CHUNKS][2]: sum |pr/s - gt/s'|, sum u . pr
    double *mapsum;      // [2B][4]  folded `part`, then [2B][2] folded `part2`
    double *img;         // [B][4]: s_pr, s_gt, 1 / (nnz + 1e-8) (0 where s_pr was clipped), D
    double *glob;        // [2]: valid count of view 1, view 2
    size_t total;
};

static PtScratch pt_carve(void *base, int B, long long N)
{
    PtScratch s;
    Carver c{base, 0};
    const size_t maps = 2 * (size_t)B;
    s.dis = c.take<float>(maps * N);
    s.mask = c.take<uint8_t>(maps * N);
    s.sel = sel_carve(c, maps);
    s.quant = c.take<float>(maps * 2);
    s.part = c.take<double>(maps * PT_MAX_CHUNKS * 4);
    s.part2 = c.take<double>(maps * PT_MAX_CHUNKS * 2);
    s.mapsum = c.take<double>(maps * 6);
    s.img = c.take<double>((size_t)B * 4);
    s.glob = c.take<double>(2);
    s.total = c.off;
    return s;
}

// workgroups per map: about 512 over the launch, at least 1 024 points each
static int pt_chunks(int B, long long N)
{
    long long c = 512 / (2LL * B), by_n = (N + 1023) / 1024;
    if (c > by_n) c = by_n;
    return (int)(c < 1 ? 1 : (c > PT_MAX_CHUNKS ? PT_MAX_CHUNKS : c));
}

__device__ inline float pt_dis(const float *__restrict__ p)
{
    const float x = p[0], y = p[1], z = p[2];
    return sqrtf(x * x + y * y + z * z);
}

// what Regr3D selects: per (view, image) map m the ranks of q = 0.002 and q = 0.998 among |gt| of all n points
struct PtSel {
    const float *gt1, *gt2;
    int B; long long n;
    float *dis, *quant, *quant_out;      // quant_out: the caller's copy, may be null
    __device__ SelPlan plan() const { return {{0.002f, 0.998f}, {SEL_ALL, SEL_ALL}}; }
    __device__ float value(int m, long long i, int pass) const
    {
        float *dm = dis + (size_t)m * n;
        if (pass) return dm[i];
        const float *gt = m < B ? gt1 + (size_t)m * n * 3 : gt2 + (size_t)(m - B) * n * 3;      // (maps: view 1's B images, then view 2's)
        return dm[i] = pt_dis(gt + 3 * i);
    }
    __device__ void finish(int m, const float *v, const float *w, bool nan) const
    {
        const float nanv = __uint_as_float(0x7fc00000u);
        const float q0 = nan ? nanv : sel_lerp(v[0], v[1], w[0]), q1 = nan ? nanv : sel_lerp(v[2], v[3], w[1]);
        quant[2 * m] = q0; quant[2 * m + 1] = q1;
        if (quant_out) { quant_out[2 * m] = q0; quant_out[2 * m + 1] = q1; }
    }
};

// ---- selection, small maps: one workgroup per map, keys in registers ----
__global__ void __launch_bounds__(SEL_ONE_BLOCK) k_sel_one(PtSel s, uint32_t *__restrict__ nanflag)
{
    __shared__ uint32_t h[SEL_RANKS * SEL_BINS];
    __shared__ uint32_t prefix[SEL_RANKS], left[SEL_RANKS];
    __shared__ uint32_t anynan;
    __shared__ float w[2];
    const SelPlan pl = s.plan();
    const int m = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const long long N = s.n;
    uint32_t key[SEL_ONE_KEYS];
    bool nan = false;
#pragma unroll
    for (int u = 0; u < SEL_ONE_KEYS; ++u) {
        const long long i = tid + (long long)u * SEL_ONE_BLOCK;
        float d = 0.f;
        if (i < N) { d = s.value(m, i, 0); nan |= d != d; }
        key[u] = sel_key(d);
    }
    if (tid == 0) anynan = 0u;
    if (tid < SEL_RANKS) {
        float wt;
        left[tid] = sel_rank((tid >> 1) ? pl.q[1] : pl.q[0], (uint32_t)N, tid & 1, &wt);
        prefix[tid] = 0u;
        if (!(tid & 1)) w[tid >> 1] = wt;
    }
    __syncthreads();
    if (nan) anynan = 1u;
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        for (int t = tid; t < SEL_RANKS * SEL_BINS; t += SEL_ONE_BLOCK) h[t] = 0u;
        __syncthreads();
        if (pass == 0) {
#pragma unroll
            for (int u = 0; u < SEL_ONE_KEYS; ++u)
                hist_bump_grouped(h, key[u] >> 24, tid + (long long)u * SEL_ONE_BLOCK < N);
        } else {
            const SelPrefixes p = sel_prefixes(prefix, 1, pass);
#pragma unroll
            for (int u = 0; u < SEL_ONE_KEYS; ++u) {
                const bool ok = tid + (long long)u * SEL_ONE_BLOCK < N;
                sel_bump_ranks(h, key[u], p, ok, ok);
            }
        }
        __syncthreads();
        if (wave < SEL_RANKS) {
            uint32_t k = left[wave];
            const uint32_t d = sel_pick(h + (pass == 0 ? 0 : wave * SEL_BINS), k);
            if ((tid & 63) == 0) { left[wave] = k; prefix[wave] |= d << (24 - 8 * pass); }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float v[SEL_RANKS] = {sel_unkey(prefix[0]), sel_unkey(prefix[1]), sel_unkey(prefix[2]), sel_unkey(prefix[3])};
        nanflag[m] = anynan;
        s.finish(m, v, w, anynan != 0u);
    }
}

// ---- reductions ----
// sum over the workgroup's 256 threads, fixed order; the total in every thread
__device__ inline double block_sum_d(double v, double *sh)
{
    v = wave_sum(v);
    __syncthreads();                                   // (sh reuse between calls)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ inline double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

struct PtArgs {
    const float *gt1, *gt2, *conf1, *conf2, *pr1, *pr2;
    long long s1, s2;          // batch strides of pr1 / pr2, in floats
    int B; long long N;
    int norm, disable_view1; float dist_clip;
};

// valid mask + per-workgroup partials: count, sum |pr|, sum |gt| over the valid points (avg_dis) or sum |pr - gt| (no normalisation)
__global__ void __launch_bounds__(PT_BLOCK) k_pt_mask(PtArgs a, const float *__restrict__ dis, const float *__restrict__ quant,
                                                      uint8_t *__restrict__ mask, uint8_t *__restrict__ valid_out, double *__restrict__ part)
{
    __shared__ double sh[4];
    const int m = blockIdx.y, view = m / a.B, b = m - view * a.B, tid = threadIdx.x;
    const long long N = a.N, per = (N + gridDim.x - 1) / gridDim.x, i0 = (long long)blockIdx.x * per, i1 = min(N, i0 + per);
    const float *gt = (view ? a.gt2 : a.gt1) + (size_t)b * N * 3, *conf = (view ? a.conf2 : a.conf1) + (size_t)b * N;
    const float *pr = view ? a.pr2 + (size_t)b * a.s2 : a.pr1 + (size_t)b * a.s1;
    const bool clip = a.dist_clip > 0.f;
    const float qlo = clip ? 0.f : quant[2 * m], qhi = clip ? 0.f : quant[2 * m + 1];
    double cnt = 0., spr = 0., sgt = 0., sl = 0.;
    for (long long i = i0 + tid; i < i1; i += PT_BLOCK) {
        bool v;
        if (clip) v = pt_dis(gt + 3 * i) <= a.dist_clip;
        else { const float d = dis[(size_t)m * N + i]; v = d >= qlo && d <= qhi && conf[i] >= CONF_MIN; }
        mask[(size_t)m * N + i] = v;
        if (valid_out) valid_out[(size_t)m * N + i] = v;
        if (v) {
            const double px = pr[3 * i], py = pr[3 * i + 1], pz = pr[3 * i + 2], gx = gt[3 * i], gy = gt[3 * i + 1], gz = gt[3 * i + 2];
            cnt += 1.;
            if (a.norm) { spr += norm3(px, py, pz); sgt += norm3(gx, gy, gz); }
            else sl += norm3(px - gx, py - gy, pz - gz);
        }
    }
    cnt = block_sum_d(cnt, sh); spr = block_sum_d(spr, sh); sgt = block_sum_d(sgt, sh); sl = block_sum_d(sl, sh);
    if (tid == 0) {
        double *p = part + ((size_t)m * PT_MAX_CHUNKS + blockIdx.x) * 4;
        p[0] = cnt; p[1] = spr; p[2] = sgt; p[3] = sl;
    }
}

// one workgroup: thread t folds map t's partials in chunk order; then the per-view counts, the per-image scales, status and (without
// normalisation) the loss
__global__ void __launch_bounds__(PT_BLOCK) k_pt_fold1(PtArgs a, int chunks, const double *__restrict__ part, const uint32_t *__restrict__ nanflag,
                                                       double *__restrict__ mapsum, double *__restrict__ img, double *__restrict__ glob,
                                                       int32_t *__restrict__ status, float *__restrict__ loss)
{
    __shared__ double cv[2];
    const int B = a.B, maps = 2 * B, tid = threadIdx.x;
    for (int m = tid; m < maps; m += PT_BLOCK) {
        double s[4] = {0., 0., 0., 0.};
        for (int c = 0; c < chunks; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] += part[((size_t)m * PT_MAX_CHUNKS + c) * 4 + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) mapsum[(size_t)m * 4 + j] = s[j];
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double c[2] = {0., 0.}, l[2] = {0., 0.};
        for (int m = 0; m < maps; ++m) { c[m / B] += mapsum[(size_t)m * 4]; l[m / B] += mapsum[(size_t)m * 4 + 3]; }
        cv[0] = glob[0] = c[0]; cv[1] = glob[1] = c[1];
        if (!a.norm) {
            const double t1 = (c[0] > 0. && !a.disable_view1) ? l[0] / c[0] : 0., t2 = c[1] > 0. ? l[1] / c[1] : 0.;
            loss[0] = (float)(t1 + t2);
        }
    }
    __syncthreads();
    for (int m = tid; m < maps; m += PT_BLOCK) {
        const double c = mapsum[(size_t)m * 4];
        status[2 * m] = (int32_t)c;
        status[2 * m + 1] = (c > 0. ? 0 : GSR_PT_EMPTY_MAP) | ((a.dist_clip > 0.f || !nanflag[m]) ? 0 : GSR_PT_NAN) | (cv[m / B] > 0. ? 0 : GSR_PT_EMPTY_VIEW);
    }
    for (int b = tid; b < B; b += PT_BLOCK) {
        const double *m1 = mapsum + (size_t)b * 4, *m2 = mapsum + (size_t)(B + b) * 4;
        const double den = m1[0] + m2[0] + 1e-8, spr = (m1[1] + m2[1]) / den, sgt = (m1[2] + m2[2]) / den;
        img[4 * b] = spr < 1e-8 ? 1e-8 : spr;
        img[4 * b + 1] = sgt < 1e-8 ? 1e-8 : sgt;
        img[4 * b + 2] = spr < 1e-8 ? 0. : 1. / den;           // (clipped scale: no gradient through it, torch's clip)
        img[4 * b + 3] = 0.;
    }
}

// avg_dis: per-workgroup partials of sum |pr / s - gt / s'| and of sum u . pr (u the unit residual), the backward's per-image term
__global__ void __launch_bounds__(PT_BLOCK) k_pt_loss_norm(PtArgs a, const uint8_t *__restrict__ mask, const double *__restrict__ img,
                                                           double *__restrict__ part2)
{
    __shared__ double sh[4];
    const int m = blockIdx.y, view = m / a.B, b = m - view * a.B, tid = threadIdx.x;
    const long long N = a.N, per = (N + gridDim.x - 1) / gridDim.x, i0 = (long long)blockIdx.x * per, i1 = min(N, i0 + per);
    const float *gt = (view ? a.gt2 : a.gt1) + (size_t)b * N * 3;
    const float *pr = view ? a.pr2 + (size_t)b * a.s2 : a.pr1 + (size_t)b * a.s1;
    const double spr = img[4 * b], sgt = img[4 * b + 1];
    double sl = 0., sd = 0.;
    for (long long i = i0 + tid; i < i1; i += PT_BLOCK) {
        if (!mask[(size_t)m * N + i]) continue;
        const double px = pr[3 * i], py = pr[3 * i + 1], pz = pr[3 * i + 2];
        const double dx = px / spr - gt[3 * i] / sgt, dy = py / spr - gt[3 * i + 1] / sgt, dz = pz / spr - gt[3 * i + 2] / sgt;
        const double l = norm3(dx, dy, dz);
        sl += l;
        if (l > 0.) sd += (dx * px + dy * py + dz * pz) / l;
    }
    sl = block_sum_d(sl, sh); sd = block_sum_d(sd, sh);
    if (tid == 0) {
        double *p = part2 + ((size_t)m * PT_MAX_CHUNKS + blockIdx.x) * 2;
        p[0] = sl; p[1] = sd;
    }
}

__global__ void __launch_bounds__(PT_BLOCK) k_pt_fold2(PtArgs a, int chunks, const double *__restrict__ part2, const double *__restrict__ glob,
                                                       double *__restrict__ mapsum2, double *__restrict__ img, float *__restrict__ loss)
{
    const int B = a.B, maps = 2 * B, tid = threadIdx.x;
    for (int m = tid; m < maps; m += PT_BLOCK) {
        double s0 = 0., s1 = 0.;
        for (int c = 0; c < chunks; ++c) { s0 += part2[((size_t)m * PT_MAX_CHUNKS + c) * 2]; s1 += part2[((size_t)m * PT_MAX_CHUNKS + c) * 2 + 1]; }
        mapsum2[(size_t)m * 2] = s0; mapsum2[(size_t)m * 2 + 1] = s1;
    }
    __threadfence_block();
    __syncthreads();
    const double w1 = (glob[0] > 0. && !a.disable_view1) ? 1. / glob[0] : 0., w2 = glob[1] > 0. ? 1. / glob[1] : 0.;
    if (tid == 0) {
        double l[2] = {0., 0.};
        for (int m = 0; m < maps; ++m) l[m / B] += mapsum2[(size_t)m * 2];
        loss[0] = (float)(l[0] * w1 + l[1] * w2);
    }
    for (int b = tid; b < B; b += PT_BLOCK) img[4 * b + 3] = w1 * mapsum2[(size_t)b * 2 + 1] + w2 * mapsum2[(size_t)(B + b) * 2 + 1];
}

// d loss / d pr: every element written (0 off the valid set)
__global__ void __launch_bounds__(PT_BLOCK) k_pt_bwd(PtArgs a, const uint8_t *__restrict__ mask, const double *__restrict__ img,
                                                     const double *__restrict__ glob, const float *__restrict__ grad_loss,
                                                     float *__restrict__ d1, float *__restrict__ d2)
{
    const int m = blockIdx.y, view = m / a.B, b = m - view * a.B, tid = threadIdx.x;
    const long long N = a.N, per = (N + gridDim.x - 1) / gridDim.x, i0 = (long long)blockIdx.x * per, i1 = min(N, i0 + per);
    const float *gt = (view ? a.gt2 : a.gt1) + (size_t)b * N * 3;
    const float *pr = view ? a.pr2 + (size_t)b * a.s2 : a.pr1 + (size_t)b * a.s1;
    float *out = (view ? d2 : d1) + (size_t)b * N * 3;
    const double g = grad_loss[0], cnt = glob[view];
    const double c = (cnt > 0. && !(view == 0 && a.disable_view1)) ? g / cnt : 0.;
    const double spr = a.norm ? img[4 * b] : 1., sgt = a.norm ? img[4 * b + 1] : 1.;
    const double through = a.norm ? g * img[4 * b + 3] / (spr * spr) * img[4 * b + 2] : 0.;      // g D / s^2 / (nnz + 1e-8)
    for (long long i = i0 + tid; i < i1; i += PT_BLOCK) {
        double ox = 0., oy = 0., oz = 0.;
        if (mask[(size_t)m * N + i]) {
            const double px = pr[3 * i], py = pr[3 * i + 1], pz = pr[3 * i + 2];
            const double dx = px / spr - gt[3 * i] / sgt, dy = py / spr - gt[3 * i + 1] / sgt, dz = pz / spr - gt[3 * i + 2] / sgt;
            const double l = norm3(dx, dy, dz);
            if (l > 0.) { const double k = c / (l * spr); ox = k * dx; oy = k * dy; oz = k * dz; }      // (0 where pr == gt: torch's norm)
            if (a.norm) {
                const double pn = norm3(px, py, pz);
                if (pn > 0.) { const double k = through / pn; ox -= k * px; oy -= k * py; oz -= k * pz; }
            }
        }
        out[3 * i] = (float)ox; out[3 * i + 1] = (float)oy; out[3 * i + 2] = (float)oz;
    }
}

// ---- teacher head post-processing ----
__global__ void __launch_bounds__(PT_BLOCK) k_pointmap_post(const float *__restrict__ raw, long long P, long long HW, float *__restrict__ pts,
                                                            float *__restrict__ conf)
{
    const long long total = P * HW;
    for (long long t = (long long)blockIdx.x * PT_BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * PT_BLOCK) {
        const long long p = t / HW, i = t - p * HW;
        const float *r = raw + (size_t)p * 4 * HW + i;
        // float64 inside: expm1 amplifies the relative error of |xyz| by |xyz| (x 20 for a far point)
        const double x = r[0], y = r[HW], z = r[2 * HW];
        const double d = norm3(x, y, z), k = expm1(d) / (d < 1e-8 ? 1e-8 : d);
        pts[3 * t] = (float)(x * k); pts[3 * t + 1] = (float)(y * k); pts[3 * t + 2] = (float)(z * k);
        conf[t] = 1.0f + expf(r[3 * HW]);
    }
}

#pragma clang fp contract(fast)

static bool pt_args_ok(const PtArgs &a)
{
    if (!a.gt1 || !a.gt2 || !a.pr1 || !a.pr2) return false;
    if (a.B < 1 || a.B > 32767 || a.N < 2 || a.N > (1LL << 31)) return false;
    return a.s1 >= 3 * a.N && a.s2 >= 3 * a.N;
}

}  // namespace gsr

extern "C" {

__attribute__((visibility("default"))) size_t gsr_regr3d_scratch_bytes(int B, int64_t N)
{
    if (B < 1 || N < 2) return 0;
    return gsr::pt_carve(nullptr, B, N).total;
}

__attribute__((visibility("default"))) int gsr_regr3d_fwd(const float *gt1, const float *gt2, const float *conf1, const float *conf2,
                                                          const float *pr1, const float *pr2, int64_t pr1_batch_stride, int64_t pr2_batch_stride,
                                                          int B, int64_t N, int norm, int disable_view1, float dist_clip, void *scratch,
                                                          float *loss, int32_t *status, float *quantiles, uint8_t *valid, void *stream)
{
    using namespace gsr;
    PtArgs a{gt1, gt2, conf1, conf2, pr1, pr2, pr1_batch_stride, pr2_batch_stride, B, N, norm, disable_view1, dist_clip};
    if (!pt_args_ok(a) || !conf1 || !conf2 || !scratch || !loss || !status || norm < 0 || norm > 1) return GSR_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PtScratch sc = pt_carve(scratch, B, N);
    const int maps = 2 * B, chunks = pt_chunks(B, N);
    (void)hipGetLastError();
    if (!(dist_clip > 0.f)) {
        const PtSel ps{gt1, gt2, B, (long long)N, sc.dis, sc.quant, quantiles};
        if (N <= SEL_ONE_MAX_N) {
            hipLaunchKernelGGL(k_sel_one, dim3(maps), dim3(SEL_ONE_BLOCK), 0, s, ps, sc.sel.nanflag);
        } else {
            if (!hip_ok(hipMemsetAsync(sc.sel.hist, 0, sel_zero_bytes(sc.sel), s))) return GSR_ELAUNCH;
            sel_run(ps, maps, chunks, sc.sel, s);
        }
    } else if (quantiles) {
        if (!hip_ok(hipMemsetAsync(quantiles, 0, (size_t)maps * 2 * 4, s))) return GSR_ELAUNCH;     // (dist_clip: no quantiles are taken)
    }
    hipLaunchKernelGGL(k_pt_mask, dim3(chunks, maps), dim3(PT_BLOCK), 0, s, a, sc.dis, sc.quant, sc.mask, valid, sc.part);
    hipLaunchKernelGGL(k_pt_fold1, dim3(1), dim3(PT_BLOCK), 0, s, a, chunks, sc.part, sc.sel.nanflag, sc.mapsum, sc.img, sc.glob, status, loss);
    if (norm) {
        hipLaunchKernelGGL(k_pt_loss_norm, dim3(chunks, maps), dim3(PT_BLOCK), 0, s, a, sc.mask, sc.img, sc.part2);
        hipLaunchKernelGGL(k_pt_fold2, dim3(1), dim3(PT_BLOCK), 0, s, a, chunks, sc.part2, sc.glob, sc.mapsum + (size_t)maps * 4, sc.img, loss);
    }
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_regr3d_bwd(const float *gt1, const float *gt2, const float *pr1, const float *pr2,
                                                          int64_t pr1_batch_stride, int64_t pr2_batch_stride, int B, int64_t N, int norm,
                                                          int disable_view1, const float *grad_loss, const void *scratch, float *grad_pr1,
                                                          float *grad_pr2, void *stream)
{
    using namespace gsr;
    PtArgs a{gt1, gt2, nullptr, nullptr, pr1, pr2, pr1_batch_stride, pr2_batch_stride, B, N, norm, disable_view1, 0.f};
    if (!pt_args_ok(a) || !grad_loss || !scratch || !grad_pr1 || !grad_pr2 || norm < 0 || norm > 1) return GSR_EINVAL;
    const PtScratch sc = pt_carve(const_cast<void *>(scratch), B, N);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pt_bwd, dim3(pt_chunks(B, N), 2 * B), dim3(PT_BLOCK), 0, static_cast<hipStream_t>(stream), a, sc.mask, sc.img, sc.glob,
                       grad_loss, grad_pr1, grad_pr2);
    return launch_status();
}

__attribute__((visibility("default"))) int gsr_pointmap_post(const float *raw, int64_t P, int H, int W, float *pts3d, float *conf, void *stream)
{
    if (!raw || !pts3d || !conf || P < 1 || H < 1 || W < 1) return GSR_EINVAL;
    const long long HW = (long long)H * W, total = (long long)P * HW;
    long long groups = (total + gsr::PT_BLOCK - 1) / gsr::PT_BLOCK;
    if (groups > 4096) groups = 4096;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gsr::k_pointmap_post, dim3((unsigned)groups), dim3(gsr::PT_BLOCK), 0, static_cast<hipStream_t>(stream), raw, (long long)P, HW,
                       pts3d, conf);
    return gsr::launch_status();
}

}  // extern "C"
