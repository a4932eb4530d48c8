// Block-streamed multi-head self-attention for sequences of up to 1024 tokens (head dim 32 / 64) on gfx950.
//
// csrc/attention.hip keeps the whole K and V of one (sequence, head) in LDS and therefore stops at 416 tokens.  Here K / V (forward,
// backward phase A) or Q / dO (backward phase B) pass through LDS in BLOCKS of KB = 128 rows, so the LDS of a workgroup does not depend
// on T.  The operand layouts are those of attention.hip (one padded image per matrix, transposed scores, P converted in place to the
// B operand of the next MFMA), and so are the pieces: operand helpers, sequence view, score tiles, the backward's tile pairs, stores and
// dbias epilogue all come from attention_pieces.h.  What is here is the block streaming (BlockRegs) and the walk over chunks and blocks.
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
// The _drop entries (dropout on the probabilities) are the same kernels with the DROP flag: the mask of (sequence, head, query, key) comes
// from csrc/dropout_pieces.h, whose grouping of eight is the eight probabilities a lane holds for one query and one 32-key chunk.
#include <type_traits>
#include "attention_pieces.h"
#include "dropout_host.h"

namespace {

constexpr int KB = 128;        // rows of a streamed block
constexpr int QC = 64;         // query (phase B: key) rows a workgroup owns at a time: one 16-row tile per wave
constexpr int NW = 4;          // waves per workgroup
constexpr int T_MAX = 1024;    // statistics rows held in LDS (a fixed size, not a function of T)

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

// S^T tiles of one 128-key block against the wave's 16 queries.
template <int HD>
__device__ __forceinline__ void block_scores(f32x4 (&s)[KB / 16], const char* kimg, const float* madd_blk, const bf16x8 (&qf)[HD / 32], int lane) {
#pragma unroll
    for (int kt = 0; kt < KB / 16; ++kt) score_tile<HD>(s[kt], kimg, madd_blk, kt, qf, lane);
}

// ------------------------------------------------------------------------------------------------ forward
template <int HD, bool DROP>
__device__ __forceinline__ void attn_stream_fwd_body(const wj_attn_fwd_args& a, int nqc, const DropParams& d) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HD / 16;
    __shared__ __attribute__((aligned(16))) char kimg[KB * RS];
    __shared__ __attribute__((aligned(16))) char vimg[KB * RS];
    __shared__ __attribute__((aligned(16))) float madd[T_MAX];    // 0 = key attended, -inf = masked / padding
    const SeqView<HD> sv(a, nqc);                                  // the chunks and heads of one sequence on one XCD (shared K / V lines)
    const int T = sv.T, D = sv.D, qc = sv.chunk;
    if (qc * QC >= T) return;            // (the whole workgroup: a chunk past the end of a short or empty sequence)
    const int nblk = (T + KB - 1) / KB;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = sv.ld;
    const bf16_t* base = sv.qkv;
    const int qt = qc * (QC / 16) + wave;                          // this wave's query tile (all padding when qt * 16 >= T: computed, never stored)
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = row_frag_global(base, ld, qt * 16, T, ks, lane, HD);
    BlockRegs<HD> nxt;
    nxt.template load<false>(base + D, ld, nullptr, 0, 0, T);
    for (int k = threadIdx.x; k < nblk * KB; k += NW * 64)
        madd[k] = (k < T && !(sv.km && sv.km[k])) ? 0.f : -INFINITY;

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
            bf16x8 pf = pack_tiles(s[2 * c], s[2 * c + 1]);
            // dropout: the dropped elements of the rounded P are zeroed; the survivors' scale goes once onto O below
            if constexpr (DROP)
                pf = DropBits{drop_keep_bits(d, drop_attn_group((uint64_t)sv.b * sv.H + sv.h, qt * 16 + i, kb * (KB / 32) + c, g)), d.scale}.mask_p(pf);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(vimg, c, dt * 16, lane), pf, o[dt], 0, 0, 0);
        }
    }
    if constexpr (DROP) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= d.scale;
    }
    store_out_lse<HD>(sv, a, qt * 16 + i, o, sum, msafe, scale, g);
}
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_fwd_kernel(wj_attn_fwd_args a, int nqc) {
    attn_stream_fwd_body<HD, false>(a, nqc, DropParams{});
}
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_fwd_drop_kernel(wj_attn_fwd_args a, int nqc, DropParams d) {
    attn_stream_fwd_body<HD, true>(a, nqc, d);
}

// ------------------------------------------------------------------------------------------------ backward
// p = exp(s * scale - lse) is recomputed per block from the stored lse; masked and padding keys carry kvalid = -inf INTO the exponent and
// padding query rows carry lse = +inf, so no product of 0 with an overflowed exp can arise (see the note in attention_pieces.h).
template <int HD, bool DROP>
__device__ __forceinline__ void attn_stream_bwd_body(const wj_attn_bwd_args& a, const DropParams& d) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HD / 16;
    using Form = BwdForm<true, true, false>;
    using DM = std::conditional_t<DROP, DropBits, NoDrop>;
    __shared__ __attribute__((aligned(16))) char img0[KB * RS];   // phase A: K block      phase B: Q block
    __shared__ __attribute__((aligned(16))) char img1[KB * RS];   // phase A: V block      phase B: dO block
    __shared__ __attribute__((aligned(16))) float lse_s[T_MAX];   // lse * log2 e (+inf for rows >= T)
    __shared__ __attribute__((aligned(16))) float delta[T_MAX];   // rowsum(dO . O)
    __shared__ __attribute__((aligned(16))) float kvalid[T_MAX];  // 0 = key attended, -inf = masked / padding (added to the exponent)
    __shared__ float bsum[NW * 3 * HD];                           // per-wave column sums of dq | dk | dv (in_proj_bias grad)
    const SeqView<HD> sv(a);                                      // heads of one sequence on one XCD
    const int T = sv.T, D = sv.D;
    const int nblk = (T + KB - 1) / KB, nqc = (T + QC - 1) / QC;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = sv.ld;
    const bf16_t *qkv = sv.qkv, *dO = sv.dO;
    const uint64_t bh = (uint64_t)sv.b * sv.H + sv.h;            // (DROP: the mask's sequence and head)

    BlockRegs<HD> nxt;
    nxt.template load<true>(qkv + D, ld, qkv + 2 * D, ld, 0, T);
    stats_rows<HD>(sv, a.lse, nblk * KB, NW * 64, lse_s, delta, kvalid);
    const float scale = rsqrtf((float)HD), scale2 = scale * LOG2E;
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase A: dQ of 16 queries per wave and chunk, K / V blocks streamed
    f32x4 csq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csq[dt] = zero4;
    for (int qc = 0; qc < nqc; ++qc) {
        const int qt = qc * (QC / 16) + wave;
        bf16x8 qf[KS], dof[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = row_frag_global(qkv, ld, qt * 16, T, ks, lane, HD);
            dof[ks] = row_frag_global(dO, D, qt * 16, T, ks, lane, HD);
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
                DM dm;
                // queries on the lane, the pair's eight keys on the accumulator rows: the forward's group, one generator call
                if constexpr (DROP) dm = DropBits{drop_keep_bits(d, drop_attn_group(bh, qt * 16 + i, kb * (KB / 32) + c, g)), d.scale};
                const bf16x8 dsf = phase_a_pair<HD, Form, DM>(img0, img1, c, KB / 16, qf, dof, kvalid + kb * KB, my_lse, my_delta, scale, scale2, lane, dm);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img0, c, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
            }
        }
        store_tile<false>(sv.dqkv, ld, qt * 16 + i, T, dq, csq, g);
    }
    if (a.dbias) bsum_add<HD, true>(bsum, 0, csq, wave, lane);

    // ---- phase B: dK, dV of 16 keys per wave and chunk, Q / dO blocks streamed
    f32x4 csk[DT], csv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csk[dt] = csv[dt] = zero4;
    if (nqc > 0) nxt.template load<true>(qkv, ld, dO, D, 0, T);
    for (int kc = 0; kc < nqc; ++kc) {
        const int kt = kc * (QC / 16) + wave;
        bf16x8 kf[KS], vf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[ks] = row_frag_global(qkv + D, ld, kt * 16, T, ks, lane, HD);
            vf[ks] = row_frag_global(qkv + 2 * D, ld, kt * 16, T, ks, lane, HD);
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
                bf16x8 pf, dsf;
                DM dm;
                if constexpr (DROP) {
                    // keys on the lane, the pair's eight QUERIES on the accumulator rows: eight groups, one draw of each (the key's)
                    const int k = kt * 16 + i, kg_c = k >> 5, kg_g = (k & 15) >> 2, j = drop_attn_draw(k);
                    uint32_t bits = 0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int q = qb * KB + c * 32 + (e >> 2) * 16 + 4 * g + (e & 3);
                        bits |= (uint32_t)(drop_draw(drop_draws(d, drop_attn_group(bh, q, kg_c, kg_g)), j) >= d.thr) << e;
                    }
                    dm = DropBits{bits, d.scale};
                }
                phase_b_pair<HD, Form, DM>(img0, img1, c, KB / 16, kf, vf, lse_s + qb * KB, delta + qb * KB, my_kv, scale, scale2, lane, pf, dsf, dm);
                if constexpr (DROP) pf = dm.mask_p(pf);      // dV += (P o m)^T dO; the scale goes once onto dV below
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img1, c, dt * 16, lane), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(img0, c, dt * 16, lane), dsf, dk[dt], 0, 0, 0);
                }
            }
        }
        if constexpr (DROP) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dv[dt] *= d.scale;
        }
        store_tile<false>(sv.dqkv + D, ld, kt * 16 + i, T, dk, csk, g);
        store_tile<false>(sv.dqkv + 2 * D, ld, kt * 16 + i, T, dv, csv, g);
    }
    if (a.dbias) {
        bsum_add<HD, true>(bsum, 1, csk, wave, lane);
        bsum_add<HD, true>(bsum, 2, csv, wave, lane);
        __syncthreads();
        // the (b, h) slice of this sequence's partial row, the waves added in wave order in both modes
        dbias_store<HD, HD, NW, true>(bsum, a.dbias_ws, sv, NW * 64);
    }
}
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_bwd_kernel(wj_attn_bwd_args a) {
    attn_stream_bwd_body<HD, false>(a, DropParams{});
}
template <int HD>
__global__ __launch_bounds__(NW * 64, 2) void attn_stream_bwd_drop_kernel(wj_attn_bwd_args a, DropParams d) {
    attn_stream_bwd_body<HD, true>(a, d);
}

}  // namespace

extern "C" int wj_attn_stream_fwd(const wj_attn_fwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    const int rc = attn_check_args(a, AttnLimits{T_MAX, 0});
    if (rc != WJ_OK) return rc;
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
    int rc = attn_check_args(a, AttnLimits{T_MAX, 0});
    if (rc != WJ_OK) return rc;
    dim3 grid(a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    if (a->hd == 64) hipLaunchKernelGGL(attn_stream_bwd_kernel<64>, grid, dim3(NW * 64), 0, st, *a);
    else hipLaunchKernelGGL(attn_stream_bwd_kernel<32>, grid, dim3(NW * 64), 0, st, *a);
    rc = attn_fold_dbias(a, stream);
    if (rc != WJ_OK) return rc;
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

#ifdef WJ_DROPOUT_LIB
extern "C" WJ_EXPORT int wj_attn_stream_fwd_drop(const wj_attn_fwd_drop_args* ad, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!ad) return WJ_ERR_ARG;
    const wj_attn_fwd_args* a = &ad->attn;
    const int rc = attn_check_args(a, AttnLimits{T_MAX, 0});
    if (rc != WJ_OK) return rc;
    DropParams d;
    if (!drop_params(ad->drop, d)) return WJ_ERR_ARG;
    const int nqc = (a->T + QC - 1) / QC;
    if ((long)a->B * a->H * nqc > 0x7fffffffL) return WJ_ERR_ARG;
    dim3 grid(a->B * a->H * nqc);
    hipStream_t st = (hipStream_t)stream;
    if (a->hd == 64) hipLaunchKernelGGL(attn_stream_fwd_drop_kernel<64>, grid, dim3(NW * 64), 0, st, *a, nqc, d);
    else hipLaunchKernelGGL(attn_stream_fwd_drop_kernel<32>, grid, dim3(NW * 64), 0, st, *a, nqc, d);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

int64_t wj_attn_bwd_drop_ws_bytes(const wj_attn_bwd_drop_args* a) { return a->attn.B * attn_dbias_row(&a->attn) * 4; }

extern "C" WJ_EXPORT int wj_attn_stream_bwd_drop(const wj_attn_bwd_drop_args* ad, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!ad) return WJ_ERR_ARG;
    const wj_attn_bwd_args* a = &ad->attn;
    int rc = attn_check_args(a, AttnLimits{T_MAX, 0});
    if (rc != WJ_OK) return rc;
    DropParams d;
    if (!drop_params(ad->drop, d)) return WJ_ERR_ARG;
    dim3 grid(a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    if (a->hd == 64) hipLaunchKernelGGL(attn_stream_bwd_drop_kernel<64>, grid, dim3(NW * 64), 0, st, *a, d);
    else hipLaunchKernelGGL(attn_stream_bwd_drop_kernel<32>, grid, dim3(NW * 64), 0, st, *a, d);
    rc = attn_fold_dbias(a, stream);
    if (rc != WJ_OK) return rc;
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
#endif
