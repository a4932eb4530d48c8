// Block-streamed multi-head self-attention for sequences of up to 1024 tokens (head dim 32 / 64) on gfx950.
//
// csrc/attention.hip keeps the whole K and V of one (sequence, head) in LDS and therefore stops at 416 tokens.  Here K / V (forward,
// backward phase A) or Q / dO (backward phase B) pass through LDS in BLOCKS of KB = 128 rows, so the LDS of a workgroup does not depend
// on T.  The operand layouts are those of attention.hip (one padded image per matrix, transposed scores, P converted in place to the
// B operand of the next MFMA); its helpers are repeated below so that attention.hip itself stays byte for byte what it was.
//   forward : TWO passes over the keys.  Pass 1 (K blocks only): row maximum m and sum l = sum exp(s - m), kept per lane over the keys
//             that lane sees and merged across the four lane groups at the end.  Pass 2 (K and V blocks): P = exp(s - m) / l, rounded to
//             bf16 AFTER the normalisation exactly as the whole-image kernel does, O^T += V^T P^T.  The second QK^T buys the rounding
//             points of the existing kernels (no per-block rescale of O, no unnormalised bf16 P), so one fp64 bound serves both.
//             Grid: (sequence, head, 64-query chunk); one 16-query tile per wave.
//   backward: one workgroup per (sequence, head) as in attention.hip, so that the dbias partials stay ONE row per sequence.
//             Phase A walks the 64-query chunks, streaming K / V blocks (dQ); phase B walks the 64-key chunks, streaming Q / dO
//             blocks (dK, dV).  Every output row has one owner: no atomics on dqkv.  The column sums for dbias are kept per wave and
//             added in wave order (what attention.hip does in its DET twins) in both modes.
// Why 128 keys per block: two images of 128 x (2 hd + 32) bytes are 40 KB at hd 64, which leaves room for three forward or two backward
// workgroups per CU; a block is four 32-row chunks = 8 score tiles = 32 fp32 registers per lane, which pass 1 holds at once to take one
// maximum and one rescale per block; 64 rows would double the barriers per key, 256 would leave one workgroup per CU.
// The next block's rows are fetched into registers while the current one is computed on (BlockRegs), as RowRegs does in attention.hip.
#include <stdlib.h>
#include "common.h"
#include "../../include/wavjepa_hip.h"

namespace {

constexpr int KB = 128;        // rows of a streamed block
constexpr int QC = 64;         // query (phase B: key) rows a workgroup owns at a time: one 16-row tile per wave
constexpr int NW = 4;          // waves per workgroup
constexpr int T_MAX = 1024;    // statistics rows held in LDS (a fixed size, not a function of T)
constexpr float LOG2E = 1.4426950408889634f;

template <int HD> struct Img {
    static constexpr int RS = HD * 2 + 32;  // padded row stride in bytes
    static constexpr int CH = HD / 8;       // 16-B chunks per row
};

// Rows [r0, r0 + KB) of one or two [T][ld] bf16 matrices (HD columns each) on their way into the padded LDS images; rows >= T are zero.
// load() issues every global load, store() parks them: the caller puts a block's compute between the two.
template <int HD>
struct BlockRegs {
    static constexpr int CH = Img<HD>::CH, RS = Img<HD>::RS, N = KB * CH / (NW * 64);
    uint4 v0[N], v1[N];

    template <bool TWO>
    __device__ __forceinline__ void load(const bf16_t* __restrict__ src0, long ld0, const bf16_t* __restrict__ src1, long ld1, int r0, int T) {
#pragma unroll
        for (int it = 0; it < N; ++it) {
            const int idx = threadIdx.x + it * (NW * 64);
            const int row = idx / CH, c = idx - row * CH;
            v0[it] = v1[it] = make_uint4(0, 0, 0, 0);
            if (r0 + row < T) {
                v0[it] = *reinterpret_cast<const uint4*>(src0 + (long)(r0 + row) * ld0 + c * 8);
                if constexpr (TWO) v1[it] = *reinterpret_cast<const uint4*>(src1 + (long)(r0 + row) * ld1 + c * 8);
            }
        }
    }
    template <bool TWO>
    __device__ __forceinline__ void store(char* img0, char* img1) const {
#pragma unroll
        for (int it = 0; it < N; ++it) {
            const int idx = threadIdx.x + it * (NW * 64);
            const int row = idx / CH, c = idx - row * CH;
            *reinterpret_cast<uint4*>(img0 + row * RS + c * 16) = v0[it];
            if constexpr (TWO) *reinterpret_cast<uint4*>(img1 + row * RS + c * 16) = v1[it];
        }
    }
};

// MFMA operand with k = head-dim: lane (i,g) gets row (rbase+i), d = ks*32 + 8g .. +7, from the LDS image.
template <int HD>
__device__ __forceinline__ bf16x8 row_frag(const char* img, int rbase, int ks, int lane) {
    const int i = lane & 15, g = lane >> 4;
    return *reinterpret_cast<const bf16x8*>(img + (rbase + i) * Img<HD>::RS + (ks * 4 + g) * 16);
}
// Same operand straight from global memory (each wave needs its own 16 rows exactly once per chunk).
__device__ __forceinline__ bf16x8 row_frag_global(const bf16_t* __restrict__ src, long ld, int rbase, int T, int ks, int lane) {
    const int i = lane & 15, g = lane >> 4;
    const int row = rbase + i;
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
    if (row < T) z = *reinterpret_cast<const bf16x8*>(src + (long)row * ld + ks * 32 + 8 * g);
    return z;
}
// MFMA A-operand with k = sequence (32-row chunk c of the image) and rows = head-dim slice [d0, d0+16), matched to a B operand
// built from two accumulator tiles: element j of lane group g is image row c*32 + (j<4 ? 4g+j : 16+4g+j-4).
template <int HD>
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int c, int d0, int lane) {
    const int i = lane & 15, g = lane >> 4, q = i >> 2, p = i & 3;
    const char* a0 = img + (c * 32 + 4 * g + q) * Img<HD>::RS + ((d0 + 4 * p) << 1);
    typedef __attribute__((address_space(3))) bf16x4 lds_b4;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(a0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(a0 + 16 * Img<HD>::RS));
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}
__device__ __forceinline__ bf16x8 pack_tiles(f32x4 lo, f32x4 hi) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) { r[e] = f2bf(lo[e]); r[4 + e] = f2bf(hi[e]); }
    return r;
}
__device__ __forceinline__ float group_max(float v) {  // over the 4 lane groups (same lane&15)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float row16_total(float v) {  // over the 16 lanes of one lane group
    v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
    return v + __shfl_xor(v, 8, 64);
}

// S^T tiles of one 128-key block against the wave's 16 queries; the 0 / -inf key mask rides in as the MFMA's C operand.
template <int HD>
__device__ __forceinline__ void block_scores(f32x4 (&s)[KB / 16], const char* kimg, const float* madd_blk, const bf16x8 (&qf)[HD / 32], int lane) {
    const int g = lane >> 4;
#pragma unroll
    for (int kt = 0; kt < KB / 16; ++kt) {
        s[kt] = *reinterpret_cast<const f32x4*>(madd_blk + kt * 16 + 4 * g);
#pragma unroll
        for (int ks = 0; ks < HD / 32; ++ks)
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(kimg, kt * 16, ks, lane), qf[ks], s[kt], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_fwd_kernel(wj_attn_fwd_args a, int nqc) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HD / 16;
    __shared__ __attribute__((aligned(16))) char kimg[KB * RS];
    __shared__ __attribute__((aligned(16))) char vimg[KB * RS];
    __shared__ __attribute__((aligned(16))) float madd[T_MAX];    // 0 = key attended, -inf = masked / padding
    const int H = a.H, D = H * HD;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);               // the chunks and heads of one sequence on one XCD (shared K / V lines)
    const int bh = wg / nqc, qc = wg - bh * nqc;
    const int b = bh / H, h = bh - b * H;
    int T = a.T;
    long row0 = (long)b * a.T;
    if (a.seq_off) {                     // ragged: this sequence's rows in the packed buffers
        row0 = a.seq_off[b];
        T = min(a.seq_off[b + 1] - (int)row0, a.T);
    }
    if (qc * QC >= T) return;            // (the whole workgroup: a chunk past the end of a short or empty sequence)
    const int nblk = (T + KB - 1) / KB;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = 3L * D;
    const bf16_t* base = (const bf16_t*)a.qkv + row0 * ld + h * HD;
    const int qt = qc * (QC / 16) + wave;                          // this wave's query tile (all padding when qt * 16 >= T: computed, never stored)
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = row_frag_global(base, ld, qt * 16, T, ks, lane);
    BlockRegs<HD> nxt;
    nxt.template load<false>(base + D, ld, nullptr, 0, 0, T);
    const uint8_t* km = a.key_mask ? a.key_mask + (long)(b / a.mask_group) * T : nullptr;
    for (int k = threadIdx.x; k < nblk * KB; k += NW * 64)
        madd[k] = (k < T && !(km && km[k])) ? 0.f : -INFINITY;

    const float scale = rsqrtf((float)HD), scale2 = scale * LOG2E;
    // ---- pass 1: m and l.  Each lane keeps a running (max, sum) over ITS keys; a block whose keys are all masked leaves both alone
    // (msafe = 0 keeps every exponent at -inf, never -inf - -inf).
    float m_run = -INFINITY, l_run = 0.f;
    for (int kb = 0; kb < nblk; ++kb) {
        __syncthreads();
        nxt.template store<false>(kimg, nullptr);
        __syncthreads();
        if (kb + 1 < nblk) nxt.template load<false>(base + D, ld, nullptr, 0, (kb + 1) * KB, T);
        f32x4 s[KB / 16];
        block_scores<HD>(s, kimg, madd + kb * KB, qf, lane);
        float bm = m_run;
#pragma unroll
        for (int kt = 0; kt < KB / 16; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) bm = fmaxf(bm, s[kt][r]);
        const float msafe = (bm == -INFINITY) ? 0.f : bm;
        const float m2 = msafe * scale2;
        float sum = l_run * __builtin_amdgcn_exp2f(fmaf(m_run, scale2, -m2));
#pragma unroll
        for (int kt = 0; kt < KB / 16; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum += __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale2, -m2));
        l_run = sum;
        m_run = bm;
    }
    const float mx = group_max(m_run);
    const float msafe = (mx == -INFINITY) ? 0.f : mx;   // fully masked row: all p = 0 (the reference yields NaN)
    const float m2 = msafe * scale2;
    const float sum = group_sum(l_run * __builtin_amdgcn_exp2f(fmaf(m_run, scale2, -m2)));
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;

    // ---- pass 2: P = exp(s - m) / l in bf16, O^T += V^T P^T
    nxt.template load<true>(base + D, ld, base + 2 * D, ld, 0, T);
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < nblk; ++kb) {
        __syncthreads();
        nxt.template store<true>(kimg, vimg);
        __syncthreads();
        if (kb + 1 < nblk) nxt.template load<true>(base + D, ld, base + 2 * D, ld, (kb + 1) * KB, T);
        f32x4 s[KB / 16];
        block_scores<HD>(s, kimg, madd + kb * KB, qf, lane);
#pragma unroll
        for (int c = 0; c < KB / 32; ++c) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[2 * c + u][r] = __builtin_amdgcn_exp2f(fmaf(s[2 * c + u][r], scale2, -m2)) * inv;
            // probabilities are normalised BEFORE the bf16 rounding (as a materialised softmax would be)
            const bf16x8 pf = pack_tiles(s[2 * c], s[2 * c + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(vimg, c, dt * 16, lane), pf, o[dt], 0, 0, 0);
        }
    }
    const int q = qt * 16 + i;
    if (q < T) {
        bf16_t* op = (bf16_t*)a.out + (row0 + q) * D + h * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = f2bf(o[dt][r]);
            *reinterpret_cast<bf16x4*>(op + dt * 16 + 4 * g) = ov;
        }
        if (a.lse && g == 0)
            a.lse[a.seq_off ? (row0 + q) * H + h : ((long)b * H + h) * T + q] = sum > 0.f ? fmaf(msafe, scale, __logf(sum)) : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// p = exp(s * scale - lse) is recomputed per block from the stored lse; masked and padding keys carry kvalid = -inf INTO the exponent and
// padding query rows carry lse = +inf, so no product of 0 with an overflowed exp can arise (see the note in attention.hip).
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_bwd_kernel(wj_attn_bwd_args a) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HD / 16;
    __shared__ __attribute__((aligned(16))) char img0[KB * RS];   // phase A: K block      phase B: Q block
    __shared__ __attribute__((aligned(16))) char img1[KB * RS];   // phase A: V block      phase B: dO block
    __shared__ __attribute__((aligned(16))) float lse_s[T_MAX];   // lse * log2 e (+inf for rows >= T)
    __shared__ __attribute__((aligned(16))) float delta[T_MAX];   // rowsum(dO . O)
    __shared__ __attribute__((aligned(16))) float kvalid[T_MAX];  // 0 = key attended, -inf = masked / padding (added to the exponent)
    __shared__ float bsum[NW * 3 * HD];                           // per-wave column sums of dq | dk | dv (in_proj_bias grad)
    const int H = a.H, D = H * HD;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);   // heads of one sequence on one XCD
    const int b = wg / H, h = wg - b * H;
    int T = a.T;
    long row0 = (long)b * a.T;
    if (a.seq_off) {
        row0 = a.seq_off[b];
        T = min(a.seq_off[b + 1] - (int)row0, a.T);
    }
    const int nblk = (T + KB - 1) / KB, nqc = (T + QC - 1) / QC;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = 3L * D;
    const bf16_t* qkv = (const bf16_t*)a.qkv + row0 * ld + h * HD;
    const bf16_t* dO = (const bf16_t*)a.dout + row0 * D + h * HD;
    const bf16_t* O = (const bf16_t*)a.out + row0 * D + h * HD;
    bf16_t* dqkv = (bf16_t*)a.dqkv + row0 * ld + h * HD;
    const uint8_t* km = a.key_mask ? a.key_mask + (long)(b / a.mask_group) * T : nullptr;

    BlockRegs<HD> nxt;
    nxt.template load<true>(qkv + D, ld, qkv + 2 * D, ld, 0, T);
    for (int r = threadIdx.x; r < nblk * KB; r += NW * 64) {
        float l = INFINITY, dl = 0.f, kv = -INFINITY;
        if (r < T) {
            l = a.lse[a.seq_off ? (row0 + r) * H + h : ((long)b * H + h) * T + r] * LOG2E;   // exp2 domain
            kv = (km && km[r]) ? -INFINITY : 0.f;
#pragma unroll
            for (int c = 0; c < HD / 8; ++c) {
                const bf16x8 x = *reinterpret_cast<const bf16x8*>(dO + (long)r * D + c * 8);
                const bf16x8 y = *reinterpret_cast<const bf16x8*>(O + (long)r * D + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) dl += bf2f(x[e]) * bf2f(y[e]);
            }
        }
        lse_s[r] = l; delta[r] = dl; kvalid[r] = kv;
    }
    const float scale = rsqrtf((float)HD), scale2 = scale * LOG2E;
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase A: dQ of 16 queries per wave and chunk (queries on the lane, keys on the accumulator rows), K / V blocks streamed
    f32x4 csq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csq[dt] = zero4;
    for (int qc = 0; qc < nqc; ++qc) {
        const int qt = qc * (QC / 16) + wave;
        bf16x8 qf[KS], dof[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = row_frag_global(qkv, ld, qt * 16, T, ks, lane);
            dof[ks] = row_frag_global(dO, D, qt * 16, T, ks, lane);
        }
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = zero4;
        for (int kb = 0; kb < nblk; ++kb) {
            __syncthreads();
            nxt.template store<true>(img0, img1);
            __syncthreads();
            const int nb = kb + 1 < nblk ? kb + 1 : 0;            // the next chunk starts over at block 0
            if (kb + 1 < nblk || qc + 1 < nqc) nxt.template load<true>(qkv + D, ld, qkv + 2 * D, ld, nb * KB, T);
            const float my_lse = lse_s[qt * 16 + i], my_delta = delta[qt * 16 + i];
#pragma unroll
            for (int c = 0; c < KB / 32; ++c) {
                f32x4 ds2[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int kt = 2 * c + u;
                    f32x4 s = zero4, dp = zero4;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img0, kt * 16, ks, lane), qf[ks], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img1, kt * 16, ks, lane), dof[ks], dp, 0, 0, 0);
                    }
                    const f32x4 kv = *reinterpret_cast<const f32x4*>(kvalid + kb * KB + kt * 16 + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], scale2, kv[r] - my_lse));
                        ds2[u][r] = p * (dp[r] - my_delta) * scale;
                    }
                }
                const bf16x8 dsf = pack_tiles(ds2[0], ds2[1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img0, c, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
            }
        }
        const int q = qt * 16 + i;
        if (q < T) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) { ov[r] = f2bf(dq[dt][r]); csq[dt][r] += bf2f(ov[r]); }
                *reinterpret_cast<bf16x4*>(dqkv + (long)q * ld + dt * 16 + 4 * g) = ov;
            }
        }
    }
    if (a.dbias) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = row16_total(csq[dt][r]);
                if (i == 0) bsum[wave * 3 * HD + dt * 16 + 4 * g + r] = v;
            }
    }

    // ---- phase B: dK, dV of 16 keys per wave and chunk (keys on the lane, queries on the accumulator rows), Q / dO blocks streamed
    f32x4 csk[DT], csv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csk[dt] = csv[dt] = zero4;
    if (nqc > 0) nxt.template load<true>(qkv, ld, dO, D, 0, T);
    for (int kc = 0; kc < nqc; ++kc) {
        const int kt = kc * (QC / 16) + wave;
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = row_frag_global(qkv + D, ld, kt * 16, T, ks, lane);
            vf[ks] = row_frag_global(qkv + 2 * D, ld, kt * 16, T, ks, lane);
        }
        f32x4 dk[DT], dv[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = zero4;
        for (int qb = 0; qb < nblk; ++qb) {
            __syncthreads();
            nxt.template store<true>(img0, img1);
            __syncthreads();
            const int nb = qb + 1 < nblk ? qb + 1 : 0;
            if (qb + 1 < nblk || kc + 1 < nqc) nxt.template load<true>(qkv, ld, dO, D, nb * KB, T);
            const float my_kv = kvalid[kt * 16 + i];
#pragma unroll
            for (int c = 0; c < KB / 32; ++c) {
                f32x4 p2[2], ds2[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int qt = 2 * c + u;
                    f32x4 s = zero4, dp = zero4;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img0, qt * 16, ks, lane), kf[ks], s, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img1, qt * 16, ks, lane), vf[ks], dp, 0, 0, 0);
                    }
                    const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb * KB + qt * 16 + 4 * g);
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta + qb * KB + qt * 16 + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[r], scale2, my_kv - l4[r]));
                        p2[u][r] = p;
                        ds2[u][r] = p * (dp[r] - d4[r]) * scale;
                    }
                }
                const bf16x8 pf = pack_tiles(p2[0], p2[1]);
                const bf16x8 dsf = pack_tiles(ds2[0], ds2[1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img1, c, dt * 16, lane), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img0, c, dt * 16, lane), dsf, dk[dt], 0, 0, 0);
                }
            }
        }
        const int key = kt * 16 + i;
        if (key < T) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                bf16x4 ok, ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ok[r] = f2bf(dk[dt][r]); ov[r] = f2bf(dv[dt][r]);
                    csk[dt][r] += bf2f(ok[r]); csv[dt][r] += bf2f(ov[r]);
                }
                *reinterpret_cast<bf16x4*>(dqkv + (long)key * ld + D + dt * 16 + 4 * g) = ok;
                *reinterpret_cast<bf16x4*>(dqkv + (long)key * ld + 2 * D + dt * 16 + 4 * g) = ov;
            }
        }
    }
    if (a.dbias) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = row16_total(csk[dt][r]), u = row16_total(csv[dt][r]);
                if (i == 0) {
                    bsum[wave * 3 * HD + HD + dt * 16 + 4 * g + r] = v;
                    bsum[wave * 3 * HD + 2 * HD + dt * 16 + 4 * g + r] = u;
                }
            }
        __syncthreads();
        // the (b, h) slice of this sequence's partial row, plain stores, the waves added in wave order
        for (int x = threadIdx.x; x < 3 * HD; x += NW * 64) {
            const int part = x / HD, d = x - part * HD;
            float tot = bsum[x];
#pragma unroll
            for (int w = 1; w < NW; ++w) tot += bsum[w * 3 * HD + x];
            a.dbias_ws[(long)b * 3 * D + part * D + h * HD + d] = tot;
        }
    }
}

}  // namespace

extern "C" int wj_attn_stream_fwd(const wj_attn_fwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || !a->qkv || !a->out) return WJ_ERR_ARG;
    if (a->B <= 0 || a->T <= 0 || a->T > T_MAX || a->H <= 0 || a->mask_group < 1) return WJ_ERR_ARG;
    if (a->seq_off && a->key_mask) return WJ_ERR_ARG;
    if (a->hd != 32 && a->hd != 64) return WJ_ERR_UNSUPPORTED;
    const int nqc = (a->T + QC - 1) / QC;
    if ((long)a->B * a->H * nqc > 0x7fffffffL) return WJ_ERR_ARG;
    dim3 grid(a->B * a->H * nqc);
    hipStream_t st = (hipStream_t)stream;
    if (a->hd == 64) hipLaunchKernelGGL(attn_stream_fwd_kernel<64>, grid, dim3(NW * 64), 0, st, *a, nqc);
    else hipLaunchKernelGGL(attn_stream_fwd_kernel<32>, grid, dim3(NW * 64), 0, st, *a, nqc);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_attn_stream_bwd(const wj_attn_bwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || !a->qkv || !a->out || !a->dout || !a->lse || !a->dqkv) return WJ_ERR_ARG;
    if (a->B <= 0 || a->T <= 0 || a->T > T_MAX || a->H <= 0 || a->mask_group < 1) return WJ_ERR_ARG;
    if (a->seq_off && a->key_mask) return WJ_ERR_ARG;
    if (a->hd != 32 && a->hd != 64) return WJ_ERR_UNSUPPORTED;
    if (a->dbias && !a->dbias_ws) return WJ_ERR_ARG;
    dim3 grid(a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    if (a->hd == 64) hipLaunchKernelGGL(attn_stream_bwd_kernel<64>, grid, dim3(NW * 64), 0, st, *a);
    else hipLaunchKernelGGL(attn_stream_bwd_kernel<32>, grid, dim3(NW * 64), 0, st, *a);
    if (a->dbias && !a->defer_fold) {
        wj_colsum_args c = {};
        c.deterministic = a->deterministic;
        c.x = a->dbias_ws; c.out = a->dbias; c.ldx = 3L * a->H * a->hd; c.M = a->B; c.N = 3 * a->H * a->hd;
        const int rc = wj_colsum_f32(&c, stream);
        if (rc != WJ_OK) return rc;
    }
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
