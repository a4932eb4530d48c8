// The pieces the streaming kernels are made of, one copy each: csrc/misc.hip (token plumbing, targets, masked loss, optimiser pass),
// denoise.hip, scene.hip, fp8.hip, noise_prep.hip, audio_prep.hip and monitor.hip (the collapse monitor, a library of its own)
// include this header.
//   conversions: to_f32x4 / to_bf16x4 -- four bf16 <-> four fp32 (f2bf: RNE)
//   walkers    : for_each_flat (the 256-thread grid-stride loop), for_each_row_col (the same over [rows][per_row])
//   bodies     : fill_token (one predictor-input piece: context feature or mask token, plus position), gelu_bwd8,
//                adamw_clip_coef / adamw_rates / adamw_update4 (the AdamW element update: misc.hip and optim.hip, a library of its own)
//   sums       : stage_wave_sum + fold4 (four wave sums, pairwise), fold_partials (a workspace of partials in one workgroup),
//                mean_sqdev (two-pass mean / centred sum of squares of a view).  fold4 and common.h's block_sum are two different
//                summation orders; every kernel keeps the one it has (tests/norm_reference.py, tests/optimizer_reference.py)
//   host       : grid_for, CheckedEntry (the entry protocol of common.h: clear the stale error, check behind the last launch)
#pragma once
#include "common.h"
#include "../../include/wavjepa_hip.h"

namespace {

// ---- conversions --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 to_f32x4(bf16x4 v) { return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])}; }
__device__ __forceinline__ bf16x4 to_bf16x4(f32x4 v) {
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
    return o;
}

// ---- walkers ------------------------------------------------------------------------------------------------------------------------
// f(i) for every i < n, 256 threads per workgroup, any grid
template <class F>
__device__ __forceinline__ void for_each_flat(long n, F f) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) f(i);
}
// f(r, c) for every r < rows, c < per_row
template <class F>
__device__ __forceinline__ void for_each_row_col(long rows, int per_row, F f) {
    for_each_flat(rows * per_row, [&](long i) {
        const int r = (int)(i / per_row);
        f(r, (int)(i - (long)r * per_row));
    });
}

// ---- bodies -------------------------------------------------------------------------------------------------------------------------
// columns c .. c + 3 of a predictor input row at time t: the context feature `src`, or (src < 0) the mask token rounded to bf16 first as
// mask_token.repeat(...).type_as(bf16 features) does; plus the position; y in fp32, yb its bf16 rounding
__device__ __forceinline__ void fill_token(const wj_scatter_fill_args& a, int src, int t, int c, f32x4& y, bf16x4& yb) {
    f32x4 tok;
    if (src >= 0) tok = to_f32x4(*reinterpret_cast<const bf16x4*>((const bf16_t*)a.ctx_feats + (long)src * a.D + c));
    else tok = to_f32x4(to_bf16x4(*reinterpret_cast<const f32x4*>(a.mask_token + c)));
    y = tok + *reinterpret_cast<const f32x4*>(a.pos + (long)t * a.D + c);
    yb = to_bf16x4(y);
}

// dpre = dpost * gelu'(pre), eight bf16 at a time
__device__ __forceinline__ bf16x8 gelu_bwd8(bf16x8 d, bf16x8 p) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(d[e]) * gelu_grad_f(bf2f(p[e])));
    return o;
}

// ---- the AdamW element update (adamw_kernel of misc.hip; adamw_groups_kernel of optim.hip, a library of its own) ----------------------
// Where an expression holds two products the compiler could contract around either (m', v', the clip's and the decay's sums), the
// multiply-add is written out as the fused operation adamw_kernel has always compiled to, so that the bits do not depend on the choice
// it makes in a given caller (a uniform factor here, a per-lane one there).  The last line, p * decay - q, holds ONE product: it is
// left to the compiler, which contracts it to fma(decay, p, -q) in both kernels (checked in the ISA; written as __builtin_fmaf the
// negation moves into the product -- the same bits, but not the instruction sequence adamw_kernel had).
// the clip coefficient from the one global sum of squares: grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))
__device__ __forceinline__ float adamw_clip_coef(const float* sumsq, float max_norm, float grad_scale) {
    float coef = grad_scale;
    if (max_norm > 0.f && sumsq) coef *= fminf(1.0f, max_norm / __builtin_fmaf(sqrtf(sumsq[0]), grad_scale, 1e-6f));
    return coef;
}
// what a learning rate and a weight decay become: the factor of p (1 - lr * wd) and the factor of m / den
__device__ __forceinline__ void adamw_rates(float lr, float weight_decay, float bc1, float& decay, float& step) {
    decay = __builtin_fmaf(-lr, weight_decay, 1.0f);
    step = lr / bc1;
}
// four elements: m, v the moving averages of the clipped gradient; p = p * decay - step * m / (sqrt(v) * rbc2 + eps)
__device__ __forceinline__ void adamw_update4(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, float coef, float decay, float step, float rbc2,
                                              float beta1, float beta2, float eps) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ge = g[e] * coef;
        m[e] = __builtin_fmaf(beta1, m[e], (1.0f - beta1) * ge);
        v[e] = __builtin_fmaf(beta2, v[e], ge * ((1.0f - beta2) * ge));
        p[e] *= decay;
        p[e] -= step * m[e] / __builtin_fmaf(rbc2, sqrtf(v[e]), eps);
    }
}

// ---- sums ---------------------------------------------------------------------------------------------------------------------------
// The four-wave order of a 256-thread workgroup: each wave's butterfly sum into w[wave], a barrier (the caller's: several sums share
// one), then (w0 + w1) + (w2 + w3).  `stride`: distance of the four terms (the column fold of scatter_fill_bwd_kernel: D).
__device__ __forceinline__ void stage_wave_sum(float v, float* w) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
}
__device__ __forceinline__ float fold4(const float* w, int stride = 1) { return (w[0] + w[stride]) + (w[2 * stride] + w[3 * stride]); }

// One workgroup of 1024 folds n partials: thread t adds ws[t], ws[t + 1024], ... in that order, then block_sum (N: the caller's index type)
template <class N>
__device__ __forceinline__ float fold_partials(const float* ws, N n, float* red) {
    float s = 0.f;
    for (N i = threadIdx.x; i < n; i += 1024) s += ws[i];
    return block_sum(s, red);
}

// Two passes of one workgroup of 1024 over the items x(0) .. x(n - 1) of a view (an item: one float or four): the mean over `count`
// elements, then the centred sum of squares, which is returned; both in block_sum's order.  Divisor and root are the caller's.
__device__ __forceinline__ float item_sum(float v) { return v; }
__device__ __forceinline__ float item_sum(f32x4 v) { return v[0] + v[1] + v[2] + v[3]; }
__device__ __forceinline__ void add_sqdev(float v, float mean, float& q) {
    const float d = v - mean;
    q += d * d;
}
__device__ __forceinline__ void add_sqdev(f32x4 v, float mean, float& q) {
#pragma unroll
    for (int e = 0; e < 4; ++e) add_sqdev(v[e], mean, q);
}
template <class N, class X>
__device__ __forceinline__ float mean_sqdev(N n, float count, X x, float* red, float& mean) {
    float s = 0.f;
    for (N i = threadIdx.x; i < n; i += 1024) s += item_sum(x(i));
    mean = block_sum(s, red) / count;
    float q = 0.f;
    for (N i = threadIdx.x; i < n; i += 1024) add_sqdev(x(i), mean, q);
    return block_sum(q, red);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// workgroups for n_items at per_block each: at least 1, at most cap
inline int grid_for(long n_items, int per_block, int cap = 8192) {
    long g = (n_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (int)(g > cap ? cap : g);
}

// The protocol of an entry point (common.h), stated once.  An entry's first statement is `const CheckedEntry entry(__func__);`, which
// discards the error this thread did not cause; it validates, launches, and returns entry.launched() behind its last launch.  The
// check exists only on the object, so no entry can have it without the clear.  An early return (argument error, empty problem) launches nothing.
struct CheckedEntry {
    const char* name;
    explicit CheckedEntry(const char* entry) : name(entry) { WJ_CLEAR_STALE_ERROR(); }
    int launched() const {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return WJ_OK;
        if (getenv("WJ_DEBUG")) fprintf(stderr, "[wavjepa_hip] %s: %s\n", name, hipGetErrorString(e));
        return WJ_ERR_LAUNCH;
    }
};

}  // namespace
