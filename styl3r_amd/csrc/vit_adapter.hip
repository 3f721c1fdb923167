// vit_adapter.hip -- the head tails and the Gaussian adapter as ONE forward and ONE backward kernel:
//   reg_dense_depth(mode='exp')          postprocess.py:22-60      xyz -> xyz / max(|xyz|, 1e-8) * expm1(|xyz|)
//   sigmoid + map_pdf_to_opacity         encoder_noposplat_multi_token_style.py:115-128,205-209
//   UnifiedGaussianAdapter.forward       gaussian_adapter.py:122-153  scales = min(0.001 softplus(s), 0.3),
//                                        q / (|q| + 1e-8), SH * sh_mask
//   build_covariance / quaternion_to_matrix   gaussians.py:8-44    Sigma = R diag(s)^2 R^T, xyzw quaternions
// plus the layout work around them (per-view cat, NCHW -> (b, v*H*W, .) transposes).  The reference (and round 1 of this
// build) runs these as ~40 element-wise framework launches forward and ~60 backward over 1-2.6 M Gaussians.
// Here: one thread per (scene, view, pixel); every head channel is read once with lane-contiguous (coalesced) loads from
// the heads' NCHW outputs, the Gaussian is assembled in registers and stored in the rasterizer's layout; the backward
// recomputes the few intermediates instead of saving them.  HBM-bound: 4 * (11 + 3 d_sh) B read + 4 * (13 + 3 d_sh) B
// written per Gaussian forward.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_common.h"
#include "vit_internal.h"

namespace vit {
struct Adp {   // per-Gaussian intermediates shared by forward and backward
    float xyz[3], d, f;          // |xyz|, expm1(|xyz|)
    float p, op;                 // sigmoid(density), mapped opacity
    float sp[3], s[3];           // softplus, clamped scale
    float q[4], n, qh[4], u;     // raw quaternion, norm, normalised, two_s
    float R[9];
};

#pragma clang fp contract(off)
__device__ inline const float *sample_ptr(const float *p0, const float *pr, int bi, int view, int v, int C, int64_t HW)
{
    return view == 0 ? p0 + (int64_t)bi * C * HW : pr + ((int64_t)bi * (v - 1) + (view - 1)) * C * HW;
}

__device__ inline void adapter_eval(const VitAdapterArgs &a, int bi, int view, int64_t r, Adp &g)
{
    const int64_t HW = (int64_t)a.H * a.W;
    const float *pt = sample_ptr(a.pts0, a.ptsr, bi, view, a.v, 3, HW) + r;
    const float *pa = sample_ptr(a.par0, a.parr, bi, view, a.v, a.par_channels, HW) + r;
#pragma unroll
    for (int c = 0; c < 3; ++c) g.xyz[c] = pt[c * HW];
    g.d = sqrtf(g.xyz[0] * g.xyz[0] + g.xyz[1] * g.xyz[1] + g.xyz[2] * g.xyz[2]);
    g.f = expm1f(g.d);
    const float dens = pa[0];
    g.p = 1.0f / (1.0f + expf(-dens));
    const float e = a.opacity_exponent;
    g.op = (e == 1.0f) ? g.p : 0.5f * (1.0f - powf(1.0f - g.p, e) + powf(g.p, 1.0f / e));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = pa[(1 + c) * HW];
        g.sp[c] = x > 20.0f ? x : log1pf(expf(x));
        g.s[c] = fminf(0.001f * g.sp[c], 0.3f);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) g.q[c] = pa[(4 + c) * HW];
    g.n = sqrtf(g.q[0] * g.q[0] + g.q[1] * g.q[1] + g.q[2] * g.q[2] + g.q[3] * g.q[3]);
    const float inv = 1.0f / (g.n + 1e-8f);
#pragma unroll
    for (int c = 0; c < 4; ++c) g.qh[c] = g.q[c] * inv;
    const float i = g.qh[0], j = g.qh[1], k = g.qh[2], w = g.qh[3];
    g.u = 2.0f / ((i * i + j * j + k * k + w * w) + 1e-8f);
    const float u = g.u;
    g.R[0] = 1.0f - u * (j * j + k * k); g.R[1] = u * (i * j - k * w); g.R[2] = u * (i * k + j * w);
    g.R[3] = u * (i * j + k * w); g.R[4] = 1.0f - u * (i * i + k * k); g.R[5] = u * (j * k - i * w);
    g.R[6] = u * (i * k - j * w); g.R[7] = u * (j * k + i * w); g.R[8] = 1.0f - u * (i * i + j * j);
}

__global__ void __launch_bounds__(256) k_adapter_fwd(VitAdapterArgs a, float *__restrict__ means, float *__restrict__ cov,
                                                     float *__restrict__ sh, float *__restrict__ opac,
                                                     float *__restrict__ scales, float *__restrict__ rot)
{
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t total = (int64_t)a.b * a.v * HW;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t r = idx % HW;
    const int view = (int)((idx / HW) % a.v), bi = (int)(idx / (HW * a.v));
    Adp g;
    adapter_eval(a, bi, view, r, g);
    const float dn = fmaxf(g.d, 1e-8f);
    float *m = means + idx * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = g.xyz[c] / dn * g.f;
    opac[idx] = g.op;
    float M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[3 * i + k] = g.R[3 * i + k] * g.s[k];
    float *S = cov + idx * 9;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[3 * i + j] = (M[3 * i] * M[3 * j] + M[3 * i + 1] * M[3 * j + 1]) + M[3 * i + 2] * M[3 * j + 2];
    if (scales) {
#pragma unroll
        for (int c = 0; c < 3; ++c) scales[idx * 3 + c] = g.s[c];
    }
    if (rot) {
#pragma unroll
        for (int c = 0; c < 4; ++c) rot[idx * 4 + c] = g.qh[c];
    }
    // SH: channel c * d_sh + k of the appearance head (or of the gs head behind its 8 structure channels) -> (3, d_sh) * mask[k]
    const int n3 = 3 * a.d_sh;
    const float *src = a.app ? a.app + ((int64_t)bi * a.v + view) * n3 * HW + r
                             : sample_ptr(a.par0, a.parr, bi, view, a.v, a.par_channels, HW) + 8 * HW + r;
    float *o = sh + idx * n3;
    for (int c = 0; c < n3; ++c) o[c] = src[c * HW] * a.sh_mask[c % a.d_sh];
}

__global__ void __launch_bounds__(256) k_adapter_bwd(VitAdapterArgs a, const float *__restrict__ d_means,
                                                     const float *__restrict__ d_cov, const float *__restrict__ d_sh,
                                                     const float *__restrict__ d_opac, float *__restrict__ d_pts0,
                                                     float *__restrict__ d_ptsr, float *__restrict__ d_par0,
                                                     float *__restrict__ d_parr, float *__restrict__ d_app)
{
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t total = (int64_t)a.b * a.v * HW;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int64_t r = idx % HW;
    const int view = (int)((idx / HW) % a.v), bi = (int)(idx / (HW * a.v));
    Adp g;
    adapter_eval(a, bi, view, r, g);
    float *gp = const_cast<float *>(sample_ptr(d_pts0, d_ptsr, bi, view, a.v, 3, HW)) + r;
    float *ga = const_cast<float *>(sample_ptr(d_par0, d_parr, bi, view, a.v, a.par_channels, HW)) + r;

    // ---- means: m = xyz * (f / dn), dn = max(d, 1e-8): dm_c/dxyz_a = delta_ca f / dn + xyz_c xyz_a coef ----
    {
        const float dn = fmaxf(g.d, 1e-8f);
        const float gm[3] = {d_means[idx * 3], d_means[idx * 3 + 1], d_means[idx * 3 + 2]};
        const float ratio = g.f / dn;
        const float dot = gm[0] * g.xyz[0] + gm[1] * g.xyz[1] + gm[2] * g.xyz[2];
        // d >= 1e-8: d(f/d)/dxyz = ((f' d - f) / d^2) * xyz / d, f' = exp(d) = f + 1.  0 < d < 1e-8: the clip holds dn at 1e-8 and only f
        // varies, d(f/dn)/dxyz = (f' / dn) * xyz / d -- as large as the first term (f ~ d).  d = 0: |xyz| has the subgradient 0 there.
        const float coef = (g.d >= 1e-8f) ? (((g.f + 1.0f) * dn - g.f) / (dn * dn)) / dn : (g.d > 0.0f) ? (g.f + 1.0f) / (dn * g.d) : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) gp[c * HW] = gm[c] * ratio + g.xyz[c] * (dot * coef);
    }
    // ---- opacity ----
    {
        const float e = a.opacity_exponent;
        const float dodp = (e == 1.0f) ? 1.0f : 0.5f * (e * powf(1.0f - g.p, e - 1.0f) + (1.0f / e) * powf(g.p, 1.0f / e - 1.0f));
        ga[0] = d_opac[idx] * dodp * (g.p * (1.0f - g.p));
    }
    // ---- covariance: Sigma = M M^T, M_ik = R_ik s_k ----
    float gS[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) gS[c] = d_cov[idx * 9 + c];
    float M[9], gM[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) M[3 * i + k] = g.R[3 * i + k] * g.s[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc += (gS[3 * i + j] + gS[3 * j + i]) * M[3 * j + k];
            gM[3 * i + k] = acc;
        }
    float gR[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float gs = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) { gs += gM[3 * i + k] * g.R[3 * i + k]; gR[3 * i + k] = gM[3 * i + k] * g.s[k]; }
        // s = min(0.001 softplus(x), 0.3): d softplus = sigmoid(x) = 1 - exp(-softplus); clamp_max passes the gradient at <= max
        const float pass = (0.001f * g.sp[k] <= 0.3f) ? 1.0f : 0.0f;
        const float raw = sample_ptr(a.par0, a.parr, bi, view, a.v, a.par_channels, HW)[r + (1 + k) * HW];
        const float dsp = raw > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-raw));
        ga[(1 + k) * HW] = gs * pass * 0.001f * dsp;
    }
    // ---- rotation: R = I + u P(qh), u = 2 / (qh.qh + eps) ----
    {
        const float i = g.qh[0], j = g.qh[1], k = g.qh[2], w = g.qh[3], u = g.u;
        const float P[9] = {-(j * j + k * k), i * j - k * w, i * k + j * w, i * j + k * w, -(i * i + k * k), j * k - i * w,
                            i * k - j * w, j * k + i * w, -(i * i + j * j)};
        float gu = 0.0f;
#pragma unroll
        for (int c = 0; c < 9; ++c) gu += gR[c] * P[c];
        float gqh[4];
        gqh[0] = u * (gR[1] * j + gR[2] * k + gR[3] * j - 2.0f * i * gR[4] - w * gR[5] + k * gR[6] + w * gR[7] - 2.0f * i * gR[8]);
        gqh[1] = u * (-2.0f * j * gR[0] + i * gR[1] + w * gR[2] + i * gR[3] + k * gR[5] - w * gR[6] + k * gR[7] - 2.0f * j * gR[8]);
        gqh[2] = u * (-2.0f * k * gR[0] - w * gR[1] + i * gR[2] + w * gR[3] - 2.0f * k * gR[4] + j * gR[5] + i * gR[6] + j * gR[7]);
        gqh[3] = u * (-k * gR[1] + j * gR[2] + k * gR[3] - i * gR[5] - j * gR[6] + i * gR[7]);
        // du/dqh_a = -u^2 qh_a
#pragma unroll
        for (int c = 0; c < 4; ++c) gqh[c] -= gu * u * u * g.qh[c];
        // qh = q / (n + eps)
        const float inv = 1.0f / (g.n + 1e-8f);
        const float dot = gqh[0] * g.q[0] + gqh[1] * g.q[1] + gqh[2] * g.q[2] + gqh[3] * g.q[3];
        const float back = (g.n > 0.0f) ? dot * inv * inv / g.n : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) ga[(4 + c) * HW] = gqh[c] * inv - g.q[c] * back;
    }
    // ---- SH ----
    const int n3 = 3 * a.d_sh;
    float *dst = a.app ? d_app + ((int64_t)bi * a.v + view) * n3 * HW + r : ga + 8 * HW;
    const float *gs = d_sh + idx * n3;
    for (int c = 0; c < n3; ++c) dst[c * HW] = gs[c] * a.sh_mask[c % a.d_sh];
}
#pragma clang fp contract(fast)

static int check(const VitAdapterArgs *a)
{
    if (!a || a->b <= 0 || a->v <= 0 || a->H <= 0 || a->W <= 0 || a->d_sh <= 0 || a->d_sh > 25) return VIT_EINVAL;
    if (!a->pts0 || !a->par0 || !a->sh_mask || (a->v > 1 && (!a->ptsr || !a->parr))) return VIT_EINVAL;
    if (a->par_channels < 8 || (!a->app && a->par_channels != 8 + 3 * a->d_sh)) return VIT_EINVAL;
    if (!(a->opacity_exponent > 0.0f)) return VIT_EINVAL;
    return VIT_OK;
}

int adapter_fwd(const VitAdapterArgs *a, float *means, float *cov, float *sh, float *opac, float *scales, float *rot, hipStream_t s)
{
    int rc = check(a);
    if (rc != VIT_OK || !means || !cov || !sh || !opac) return VIT_EINVAL;
    const int64_t total = (int64_t)a->b * a->v * a->H * a->W;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_adapter_fwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *a, means, cov, sh, opac, scales, rot);
    return launch_status();
}

int adapter_bwd(const VitAdapterArgs *a, const float *d_means, const float *d_cov, const float *d_sh, const float *d_opac,
                float *d_pts0, float *d_ptsr, float *d_par0, float *d_parr, float *d_app, hipStream_t s)
{
    int rc = check(a);
    if (rc != VIT_OK || !d_means || !d_cov || !d_sh || !d_opac || !d_pts0 || !d_par0) return VIT_EINVAL;
    if (a->v > 1 && (!d_ptsr || !d_parr)) return VIT_EINVAL;
    if (a->app && !d_app) return VIT_EINVAL;
    const int64_t total = (int64_t)a->b * a->v * a->H * a->W;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_adapter_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *a, d_means, d_cov, d_sh, d_opac,
                       d_pts0, d_ptsr, d_par0, d_parr, d_app);
    return launch_status();
}

}  // namespace vit
