// The pieces the conv front-end kernels are made of, one copy each: csrc/conv0.hip (layer 0 with GroupNorm) and csrc/conv_ln.hip
// (mode="layer_norm", layer 0 and layers >= 1) include this header.
//   taps      : tap_at, tap_map, tap_offsets -- tap q = ci * k + kk of a row sits ci * pitch + kk elements from the row's first sample;
//               the pitch is the staged span (LDS chunks of conv0.hip) or the clip length L (global audio)
//   operands  : stage_chunk (a chunk's samples into LDS, bf16 or fp32, zero past the clip), load_weights, load_patch
//   arithmetic: conv_row (patch x weights, optional bias, bf16 rounding), gn_stats (GroupNorm mean / rstd from the folded sums)
//   folds     : ordered_fold_kernel / fold_records -- sum a group's partial records in record order (float or double)
//   host      : taps_dispatch / taps_ok, packed_clip_stride, row_grid
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// ---- taps ---------------------------------------------------------------------------------------------------------------------------
// offset (elements from the row's first sample) of tap q
__device__ __forceinline__ int tap_at(int q, int k, int pitch) {
    const int ci = q / k;
    return ci * pitch + (q - ci * k);
}
// the same, and ok = q < TAPS (MFMA operands pad the tap axis)
template <int TAPS>
__device__ __forceinline__ int tap_at(int q, int k, int pitch, bool& ok) {
    ok = q < TAPS;
    return tap_at(q, k, pitch);
}
// taps q0, q0 + dq, ... (NQ of them)
template <int TAPS, int NQ>
__device__ __forceinline__ void tap_map(int (&off)[NQ], bool (&ok)[NQ], int q0, int dq, int k, int pitch) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) off[j] = tap_at<TAPS>(q0 + j * dq, k, pitch, ok[j]);
}
template <int TAPS>
__device__ __forceinline__ void tap_offsets(int (&off)[TAPS], int k, int pitch) {
    bool ok[TAPS];
    tap_map<TAPS>(off, ok, 0, 1, k, pitch);
}

// ---- operands -----------------------------------------------------------------------------------------------------------------------
// xs[ci][i] = audio[clip + ci * L + s0 + i] for i < span, 0 past the clip's L samples (NT threads; T = bf16_t or float)
template <int NT, class T>
__device__ __forceinline__ void stage_chunk(T* xs, const bf16_t* __restrict__ audio, long clip, int C_in, int L, long s0, int span) {
    for (int ci = 0; ci < C_in; ++ci)
        for (int i = threadIdx.x; i < span; i += NT) {
            const long src = s0 + i;
            xs[ci * span + i] = src < L ? (T)audio[clip + (long)ci * L + src] : (T)0.f;
        }
}

// the NCH x TAPS weights of channels c0 .. c0 + NCH - 1
template <int NCH, int TAPS>
__device__ __forceinline__ void load_weights(float (&w)[NCH][TAPS], const bf16_t* __restrict__ wsrc, int c0) {
#pragma unroll
    for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int q = 0; q < TAPS; ++q) w[j][q] = bf2f(wsrc[(long)(c0 + j) * TAPS + q]);
}

// one row's patch: row = the row's first sample (LDS floats or global bf16)
template <int TAPS, class T>
__device__ __forceinline__ void load_patch(float (&x)[TAPS], const T* row, const int (&off)[TAPS]) {
#pragma unroll
    for (int q = 0; q < TAPS; ++q) x[q] = (float)row[off[q]];
}

// ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
// y[j] = bf16(sum_q x[q] w(j, q) [+ bias[j]]): the FMA chain from q = 0, then the bias, then the rounding -- the conv output is a bf16
// tensor in the reference's autocast flow.  w(j, q) reads the kernel's own weight container; bias == nullptr: no bias term.
template <int NCH, int TAPS, class W>
__device__ __forceinline__ void conv_row(float (&y)[NCH], const float (&x)[TAPS], W&& w, const float* bias) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < TAPS; ++q) a = fmaf(x[q], w(j, q), a);
        y[j] = bf2f(f2bf(bias ? a + bias[j] : a));
    }
}

// GroupNorm statistics of one (clip, channel) from its folded sum and sum of squares: one-pass variance, clamped at 0
__device__ __forceinline__ void gn_stats(float s1, float s2, float invL, float eps, float& mu, float& rstd) {
    mu = s1 * invL;
    const float var = fmaxf(s2 * invL - mu * mu, 0.f);
    rstd = rsqrtf(var + eps);
}

// ---- folds --------------------------------------------------------------------------------------------------------------------------
// out[n][i] = sum over records (in record order) of part[n][record][i]; the record is split over up to three outputs
// ([0, n0) -> o0, [n0, n0 + n1) -> o1, the rest -> o2, each [N][.]).  cnt_off != NULL: group n only has
// ceil((cnt_off[n+1] - cnt_off[n]) / per_chunk) records written (sparse backward), else `chunks`.  No float atomics: the sums are
// bit-reproducible from run to run.
template <class T>
__global__ __launch_bounds__(256) void ordered_fold_kernel(const T* __restrict__ part, int chunks, long rec, T* __restrict__ o0, long n0,
                                                           T* __restrict__ o1, long n1, T* __restrict__ o2,
                                                           const int32_t* __restrict__ cnt_off, int per_chunk) {
    const int n = blockIdx.y;
    int nch = chunks;
    if (cnt_off) nch = min(chunks, (cnt_off[n + 1] - cnt_off[n] + per_chunk - 1) / per_chunk);
    const T* src = part + (long)n * chunks * rec;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < rec; i += (long)gridDim.x * 256) {
        T s = 0;
        for (int ch = 0; ch < nch; ++ch) s += src[ch * rec + i];
        if (i < n0) o0[n * n0 + i] = s;
        else if (i < n0 + n1) o1[n * n1 + (i - n0)] = s;
        else o2[n * (rec - n0 - n1) + (i - n0 - n1)] = s;
    }
}
// grid_x workgroups per group; without the split everything goes to o0
template <class T>
void fold_records(hipStream_t s, unsigned grid_x, int groups, const T* part, int chunks, long rec, T* o0, long n0, T* o1 = nullptr,
                  long n1 = 0, T* o2 = nullptr, const int32_t* cnt_off = nullptr, int per_chunk = 1) {
    hipLaunchKernelGGL(ordered_fold_kernel<T>, dim3(grid_x, groups), dim3(256), 0, s, part, chunks, rec, o0, n0, o1, n1, o2, cnt_off, per_chunk);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// f(tap-count constant) for the supported C_in * k; false: not supported
template <class F>
bool taps_dispatch(int taps, F&& f) {
    switch (taps) {
        case 10: f(std::integral_constant<int, 10>{}); return true;
        case 20: f(std::integral_constant<int, 20>{}); return true;
        default: return false;
    }
}
inline bool taps_ok(int taps) { return taps_dispatch(taps, [](auto) {}); }

// elements between consecutive clips of the audio: 0 = packed (C_in * L); larger for one channel of a multi-channel batch
// (wavjepa/extractors/audio_channel_feature_extractor.py:163-172 runs x[:, [c]])
inline long packed_clip_stride(long clip_stride, int C_in, int L) { return clip_stride > 0 ? clip_stride : (long)C_in * L; }

// workgroups for `rows` rows at per_wg rows each; beyond the cap the kernels stride over the rows
inline unsigned row_grid(long rows, int per_wg, int cap = 8192) {
    const long grid = (rows + per_wg - 1) / per_wg;
    return (unsigned)(grid > cap ? cap : grid);
}

}  // namespace
