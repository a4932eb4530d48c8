// Shared device helpers for the gfx950 (MI355X, CDNA4) kernels of libwavjepa_hip.so.
// Wavefront = 64 lanes everywhere in this tree; nothing here is portable to 32-wide hardware.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

#define WJ_OK 0
#define WJ_ERR_ARG (-1)
#define WJ_ERR_LAUNCH (-2)
#define WJ_ERR_UNSUPPORTED (-3)

// What a library built with -fvisibility=hidden exports (the side libraries: the entries of libwavjepa_hip.so that their shared sources
// also define stay inside them); without the flag it changes nothing.
#define WJ_EXPORT __attribute__((visibility("default")))

// hipGetLastError() reports the last error of ANY HIP call of this thread -- including benign ones of the host framework (an
// event query returning hipErrorNotReady) -- so every entry point first discards what it did not cause.
#define WJ_CLEAR_STALE_ERROR() (void)hipGetLastError()

#define WJ_CHECK_LAUNCH()                                                                              \
    do {                                                                                               \
        hipError_t e__ = hipGetLastError();                                                            \
        if (e__ != hipSuccess) {                                                                       \
            if (getenv("WJ_DEBUG")) fprintf(stderr, "[wavjepa_hip] %s: %s\n", __func__, hipGetErrorString(e__)); \
            return WJ_ERR_LAUNCH;                                                                      \
        }                                                                                              \
    } while (0)

// Laboratory switches (A/B runs, diagnostics that change results or schedules): read from the environment ONLY in the -DWJ_LAB build
// (libwavjepa_hip_lab.so, include/wavjepa_hip_lab.h); the release library compiles each to its default -- a production process cannot be
// pushed onto a diagnostic path by a stray variable.  Switches that are safe in production use getenv directly and are listed in
// INTEGRATION.md (tests/test_host_cpu.py checks both lists against the sources).
#ifdef WJ_LAB
constexpr bool WJ_LAB_BUILD = true;
static inline int wj_lab_env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
static inline const char* wj_lab_env_str(const char* name) { return getenv(name); }
#else
constexpr bool WJ_LAB_BUILD = false;
static inline int wj_lab_env_int(const char*, int dflt) { return dflt; }
static inline const char* wj_lab_env_str(const char*) { return nullptr; }
#endif

// Most partial rows ([rows][3][D] floats: dgamma | dbeta | dbias) a LayerNorm backward leaves in its workspace: the grid cap of
// wj_layernorm_bwd / wj_layernorm_pre_bwd (norm.hip) and of wj_conv_ln_gelu_bwd (conv_ln.hip), whose callers hold the same scratch,
// and the size wj_workspace_bytes answers for the first two.
constexpr int LN_BWD_MAX_PARTIAL_ROWS = 1536;

__device__ __forceinline__ float bf2f(bf16_t x) { return (float)x; }
__device__ __forceinline__ bf16_t f2bf(float x) { return (bf16_t)x; }  // v_cvt_pk_bf16_f32: RNE, NaN-preserving

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x <= 1024 (<= 16 waves).  `red` is >= 16 floats of LDS.  All threads get the result.
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// erf-GELU (nn.GELU(approximate='none')) and its derivative, fp32.
// erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, far below bf16 resolution): ~14 VALU ops instead of libm's
// branchy erff (~60), and gelu' reuses the same exponential: exp(-(x/sqrt2)^2) = exp(-x^2/2).
__device__ __forceinline__ void erf_parts(float x, float& erf_abs, float& e) {
    // returns erf(|x|/sqrt2) and e = exp(-x^2/2)
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));   // v_rcp_f32 (1 ulp); __frcp_rn is a ~10-instruction IEEE divide
    e = __expf(-z * z);
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    erf_abs = fmaf(-p * t, e, 1.0f);
}
__device__ __forceinline__ float gelu_f(float x) {
    float ea, e;
    erf_parts(x, ea, e);
    return 0.5f * x * (1.0f + copysignf(ea, x));
}
// gelu(x) and gelu'(x) from one erf / one exp
__device__ __forceinline__ void gelu_both_f(float x, float& g, float& gp) {
    float ea, e;
    erf_parts(x, ea, e);
    const float cdf = 0.5f * (1.0f + copysignf(ea, x));
    g = x * cdf;
    gp = fmaf(x * 0.39894228040143267794f, e, cdf);
}
__device__ __forceinline__ float gelu_grad_f(float x) {
    float ea, e;
    erf_parts(x, ea, e);
    return fmaf(x * 0.39894228040143267794f, e, 0.5f * (1.0f + copysignf(ea, x)));
}

// The same erf-GELU written two elements at a time: left to itself hipcc packs part of the scalar form above and shuffles
// registers around it (206 VALU instructions per 8 outputs of gelu + gelu' in the GEMM epilogue, 103 written this way; 141 -> 90
// for gelu alone).  Measured: BIAS_GELU2 -6 %, CONV_GELU -4 %, conv0 apply -6 %, teacher BIAS_GELU unchanged -- on gfx950 a
// v_pk_fma_f32 issues at the cost of two v_fma_f32, so what is saved is the shuffling, not half of the arithmetic.
// Same A-S 7.1.26 erf; exp(-x^2/2) taken as exp2(x^2 * (-log2(e)/2)).
template <bool WANT_GRAD>
__device__ __forceinline__ void gelu_pk(const f32x2 x, f32x2& g, f32x2& gp) {
    constexpr float C = 0.3275911f * 0.70710678118654752440f;
    f32x2 t, e;
    t.x = __builtin_amdgcn_rcpf(fmaf(fabsf(x.x), C, 1.0f));            // |x| is a free source modifier of the scalar fma only
    t.y = __builtin_amdgcn_rcpf(fmaf(fabsf(x.y), C, 1.0f));
    const f32x2 u = (x * x) * (-0.5f * 1.44269504088896340736f);
    e.x = __builtin_amdgcn_exp2f(u.x);
    e.y = __builtin_amdgcn_exp2f(u.y);
    f32x2 p = __builtin_elementwise_fma(t, f32x2{1.061405429f, 1.061405429f}, f32x2{-1.453152027f, -1.453152027f});
    p = __builtin_elementwise_fma(p, t, f32x2{1.421413741f, 1.421413741f});
    p = __builtin_elementwise_fma(p, t, f32x2{-0.284496736f, -0.284496736f});
    p = __builtin_elementwise_fma(p, t, f32x2{0.254829592f, 0.254829592f});
    const f32x2 ea = __builtin_elementwise_fma(-(p * t), e, f32x2{1.0f, 1.0f});
    f32x2 s;
    s.x = __builtin_copysignf(ea.x, x.x);
    s.y = __builtin_copysignf(ea.y, x.y);
    const f32x2 cdf = __builtin_elementwise_fma(s, f32x2{0.5f, 0.5f}, f32x2{0.5f, 0.5f});
    g = x * cdf;
    if constexpr (WANT_GRAD) gp = __builtin_elementwise_fma(x * 0.39894228040143267794f, e, cdf);
}
// 8 bf16 in, gelu (and gelu') as 8 bf16 out
template <bool WANT_GRAD>
__device__ __forceinline__ void gelu_bf16x8(const bf16x8 h, bf16x8& g, bf16x8& gp) {
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_;
    const u32x4_ w = __builtin_bit_cast(u32x4_, h);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2 x, a, b;
        x.x = __uint_as_float(w[j] << 16);
        x.y = __uint_as_float(w[j] & 0xffff0000u);
        gelu_pk<WANT_GRAD>(x, a, b);
        g[2 * j] = f2bf(a.x); g[2 * j + 1] = f2bf(a.y);
        if constexpr (WANT_GRAD) { gp[2 * j] = f2bf(b.x); gp[2 * j + 1] = f2bf(b.y); }
    }
}

// The other feed-forward activations of linear1's epilogues (libwavjepa_hip_act.so, include/wavjepa_hip_act.h: the values of wj_act),
// two elements at a time like gelu_pk: act(h) and act'(h) in fp32 from the bf16 h, as torch defines them on a bf16 tensor.
// EVERY finite bf16 h gives finite outputs, and beyond saturation act' is exactly 1 / 0:
//   relu       (h < 0) ? 0 : h and (h > 0) ? 1 : 0: two compares, two selects; -0 stays -0 and NaN passes, as torch.relu on a bf16
//              tensor; act' = 0 at h == 0 (torch's threshold_backward).
//   silu       s = 1 / (1 + exp(-h)) as v_rcp_f32(1 + v_exp_f32(-h log2 e)).  exp overflows to +inf (h < -88.7) -> s = +0 exactly,
//              underflows to 0 (h > 104) -> s = 1 exactly; act = h s, act' = s + (h s)(1 - s) as one fma: with s in {0, 1} that is
//              fma(-0, 1, 0) = 0 or fma(h, 0, 1) = 1, no 0 * inf anywhere (h s is finite: |h s| <= |h|).
//   gelu_tanh  0.5 (1 + tanh(u)) = 1 / (1 + exp(-2u)) =: s, u = c (h + 0.044715 h^3): the same exp / rcp pair, no tanh.  act = h s,
//              act' = s + s (1 - s) . 2c h (1 + 0.134145 h^2) (1 - tanh^2 = 4 s (1 - s)).  h^2, h^3 and the polynomial are taken of
//              hc = med3(h, -16, 16): at |h| = 16 the exponent is -+459, far outside fp32, so s and s (1 - s) are exactly what they
//              are for every larger |h|, and nothing but the exp ever leaves the finite range.  act = h s uses the unclamped h.
// VALU instructions per 8 outputs of act' + act / of act alone, counted around act_bf16x8 in a stand-alone kernel (unpack and the
// bf16 conversions included), and the VGPRs of the persistent BIAS_GELU2 kernel (tools/kernel_resources.py on the -DWJ_ACT_LIB build):
// gelu_pk 98 / 86, 225;  relu 49 / 29, 222;  gelu_tanh 84 / 59, 226;  silu 53 / 41, 225.  The 256 x 128 and eight-phase kernels hold
// 108 and 228 VGPRs for every kind.  ("Feed-forward activation".)
constexpr int ACT_GELU = 0, ACT_RELU = 1, ACT_GELU_TANH = 2, ACT_SILU = 3;    // = wj_act (include/wavjepa_hip_act.h)
constexpr int ACT_KINDS = 4;

template <bool WANT_GRAD>
__device__ __forceinline__ void relu_pk(const f32x2 x, f32x2& g, f32x2& gp) {
    g.x = x.x < 0.f ? 0.f : x.x;
    g.y = x.y < 0.f ? 0.f : x.y;
    if constexpr (WANT_GRAD) {
        gp.x = x.x > 0.f ? 1.f : 0.f;
        gp.y = x.y > 0.f ? 1.f : 0.f;
    }
}
template <bool WANT_GRAD>
__device__ __forceinline__ void silu_pk(const f32x2 x, f32x2& g, f32x2& gp) {
    const f32x2 u = x * (-1.44269504088896340736f);
    f32x2 e, s;
    e.x = __builtin_amdgcn_exp2f(u.x);
    e.y = __builtin_amdgcn_exp2f(u.y);
    const f32x2 d = e + 1.0f;
    s.x = __builtin_amdgcn_rcpf(d.x);
    s.y = __builtin_amdgcn_rcpf(d.y);
    g = x * s;
    if constexpr (WANT_GRAD) gp = __builtin_elementwise_fma(g, 1.0f - s, s);
}
template <bool WANT_GRAD>
__device__ __forceinline__ void gelu_tanh_pk(const f32x2 x, f32x2& g, f32x2& gp) {
    constexpr float C2 = 2.0f * 0.79788456080286535588f;                 // 2 sqrt(2 / pi)
    constexpr float KE = -C2 * 1.44269504088896340736f;                  // exp(-2u) = exp2(KE hc (1 + 0.044715 hc^2))
    f32x2 hc, e, s;
    hc.x = __builtin_amdgcn_fmed3f(x.x, -16.0f, 16.0f);
    hc.y = __builtin_amdgcn_fmed3f(x.y, -16.0f, 16.0f);
    const f32x2 q = hc * hc;
    const f32x2 a = hc * __builtin_elementwise_fma(q, f32x2{KE * 0.044715f, KE * 0.044715f}, f32x2{KE, KE});
    e.x = __builtin_amdgcn_exp2f(a.x);
    e.y = __builtin_amdgcn_exp2f(a.y);
    const f32x2 d = e + 1.0f;
    s.x = __builtin_amdgcn_rcpf(d.x);
    s.y = __builtin_amdgcn_rcpf(d.y);
    g = x * s;
    if constexpr (WANT_GRAD) {
        const f32x2 w = hc * __builtin_elementwise_fma(q, f32x2{C2 * 0.134145f, C2 * 0.134145f}, f32x2{C2, C2});
        gp = __builtin_elementwise_fma(s * (1.0f - s), w, s);
    }
}
template <int ACT, bool WANT_GRAD>
__device__ __forceinline__ void act_pk(const f32x2 x, f32x2& g, f32x2& gp) {
    static_assert(ACT >= 0 && ACT < ACT_KINDS, "activation kind");
    if constexpr (ACT == ACT_RELU) relu_pk<WANT_GRAD>(x, g, gp);
    else if constexpr (ACT == ACT_GELU_TANH) gelu_tanh_pk<WANT_GRAD>(x, g, gp);
    else if constexpr (ACT == ACT_SILU) silu_pk<WANT_GRAD>(x, g, gp);
    else gelu_pk<WANT_GRAD>(x, g, gp);
}
// 8 bf16 in, act (and act') as 8 bf16 out; ACT_GELU is gelu_bf16x8 itself
template <int ACT, bool WANT_GRAD>
__device__ __forceinline__ void act_bf16x8(const bf16x8 h, bf16x8& g, bf16x8& gp) {
    if constexpr (ACT == ACT_GELU) {
        gelu_bf16x8<WANT_GRAD>(h, g, gp);
    } else {
        typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_;
        const u32x4_ w = __builtin_bit_cast(u32x4_, h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x2 x, a, b;
            x.x = __uint_as_float(w[j] << 16);
            x.y = __uint_as_float(w[j] & 0xffff0000u);
            act_pk<ACT, WANT_GRAD>(x, a, b);
            g[2 * j] = f2bf(a.x); g[2 * j + 1] = f2bf(a.y);
            if constexpr (WANT_GRAD) { gp[2 * j] = f2bf(b.x); gp[2 * j + 1] = f2bf(b.y); }
        }
    }
}

// XCD-aware bijective remap of a linear workgroup id: blocks b and b+8 share an XCD (round-robin dispatch),
// so give each XCD a contiguous chunk of the logical id space (neighbouring tiles then share that XCD's L2).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
