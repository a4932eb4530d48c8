// The pieces the attention kernels are made of, one copy each: csrc/attention.hip (whole K / V images in LDS, T <= 416) and
// csrc/attention_stream.hip (128-row blocks, T <= 1024) include this header and differ only in how rows reach the LDS images.
//   operands   : Img, row_frag, row_frag_global, tr_frag, pack_tiles, group_max, group_sum, row16_sum
//   sequence   : SeqView -- (b, h), T / row0 of the dense or ragged form, base pointers, key-mask row, lse index
//   forward    : score_tile, store_out_lse
//   backward   : stats_rows, phase_a_pair, phase_b_pair, store_tile, bsum_zero / bsum_add / dbias_store; the three families
//                (general, frag, streamed) name their differences in a BwdForm
//   host       : LDS byte counts, argument validation and the dbias fold of the four entry points
#pragma once
#include <stdlib.h>
#include "common.h"
#include "../../include/wavjepa_hip.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

template <int HD> struct Img {
    static constexpr int RS = HD * 2 + 32;  // padded row stride in bytes
    static constexpr int CH = HD / 8;       // 16-B chunks per row
};

// MFMA operand with k = head-dim: lane (i,g) gets row (rbase+i), d = ks*32 + 8g .. +7, from the LDS image.
template <int HD>
__device__ __forceinline__ bf16x8 row_frag(const char* img, int rbase, int ks, int lane) {
    const int i = lane & 15, g = lane >> 4;
    return *reinterpret_cast<const bf16x8*>(img + (rbase + i) * Img<HD>::RS + (ks * 4 + g) * 16);
}
// Same operand straight from global memory (each wave needs its own 16 rows exactly once); columns >= hg are zero.
__device__ __forceinline__ bf16x8 row_frag_global(const bf16_t* __restrict__ src, long ld, int rbase, int T, int ks, int lane, int hg) {
    const int i = lane & 15, g = lane >> 4;
    const int row = rbase + i;
    bf16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
    if (row < T && ks * 32 + 8 * g < hg) z = *reinterpret_cast<const bf16x8*>(src + (long)row * ld + ks * 32 + 8 * g);
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
// Sum over the 16 lanes of a DPP row (same lane >> 4), every lane gets the total: four v_add_f32 with DPP operands (quad swaps,
// then half-row and row mirrors -- once a quad holds its sum in all four lanes any pairing of quads will do) instead of four
// ds_bpermute round trips through the LDS pipe.  The partial sums pair up as in a __shfl_xor 1 / 2 / 4 / 8 butterfly, so the
// total has that butterfly's bits.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, false));  // row_mirror
    return v;
}

// ------------------------------------------------------------------------------------------------ sequence view
// What a workgroup knows about its (sequence, head), filled once at kernel entry.  HG: the head width in memory.  `chunks`: the
// workgroups that share one (sequence, head) (the streamed forward's query chunks); this one's is `chunk`.
template <int HG>
struct SeqView {
    int b, h, H, D, T, chunk;
    long row0, ld;                  // first row in the packed buffers; row stride of qkv / dqkv
    bool ragged;
    const bf16_t *qkv, *dO, *O;     // at (row0, head h): q columns of qkv, dout, out
    bf16_t* dqkv;
    const uint8_t* km;              // this sequence's key-mask row, or null

    __device__ __forceinline__ SeqView(const wj_attn_fwd_args& a, int chunks = 1) { init(a, chunks); }
    __device__ __forceinline__ SeqView(const wj_attn_bwd_args& a) {
        init(a, 1);
        dO = (const bf16_t*)a.dout + row0 * D + h * HG;
        O = (const bf16_t*)a.out + row0 * D + h * HG;
        dqkv = (bf16_t*)a.dqkv + row0 * ld + h * HG;
    }
    // lse is [B][H][T] in the dense forms and [rows][H] in the ragged one
    __device__ __forceinline__ long lse_index(int row) const { return ragged ? (row0 + row) * H + h : ((long)b * H + h) * T + row; }

private:
    template <class Args>
    __device__ __forceinline__ void init(const Args& a, int chunks) {
        H = a.H;
        D = H * HG;
        ld = 3L * D;
        // the heads of one sequence read interleaved 2*HD-byte slices of the same rows: keep them on ONE XCD so that the
        // other half of every 128-B line is an L2 hit (round-robin dispatch would spread them over all eight L2s: PMC showed
        // the hd = 32 predictor fetching 1.8x (fwd) / 2.6x (bwd) its algorithmic bytes)
        const int wg = xcd_remap(blockIdx.x, gridDim.x);
        const int bh = wg / chunks;
        chunk = wg - bh * chunks;
        b = bh / H;
        h = bh - b * H;
        T = a.T;
        row0 = (long)b * a.T;
        ragged = a.seq_off != nullptr;
        if (a.seq_off) {                     // ragged: this sequence's rows in the packed buffers
            row0 = a.seq_off[b];
            T = min(a.seq_off[b + 1] - (int)row0, a.T);
        }
        qkv = (const bf16_t*)a.qkv + row0 * ld + h * HG;
        dO = O = nullptr;
        dqkv = nullptr;
        km = a.key_mask ? a.key_mask + (long)(b / a.mask_group) * T : nullptr;
    }
};

// ------------------------------------------------------------------------------------------------ forward pieces
// One S^T tile: 16 keys of the image against the wave's 16 queries.  The 0 / -inf key mask rides in as the MFMA's C operand.
// (A wave-uniform branch that skipped the mask on tiles without one put a taken branch between an MFMA and the first VALU read of its
// result; hipcc left one wait state there and the kernel returned run-dependent sums.)
template <int HD>
__device__ __forceinline__ void score_tile(f32x4& s, const char* kimg, const float* madd, int kt, const bf16x8 (&qf)[HD / 32], int lane) {
    s = *reinterpret_cast<const f32x4*>(madd + kt * 16 + 4 * (lane >> 4));
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(kimg, kt * 16, ks, lane), qf[ks], s, 0, 0, 0);
}
// Query row q of the O^T accumulators, and its lse = max * scale + log(sum) (+inf for a row without an attended key).
template <int HG>
__device__ __forceinline__ void store_out_lse(const SeqView<HG>& sv, const wj_attn_fwd_args& a, int q, const f32x4 (&o)[HG / 16], float sum,
                                              float msafe, float scale, int g) {
    if (q < sv.T) {
        bf16_t* op = (bf16_t*)a.out + (sv.row0 + q) * sv.D + sv.h * HG;
#pragma unroll
        for (int dt = 0; dt < HG / 16; ++dt) {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = f2bf(o[dt][r]);
            *reinterpret_cast<bf16x4*>(op + dt * 16 + 4 * g) = ov;
        }
        if (a.lse && g == 0) a.lse[sv.lse_index(q)] = sum > 0.f ? fmaf(msafe, scale, __logf(sum)) : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------------ backward pieces
// Masked and padding keys in the backward.  Every backward kernel recomputes p = exp(s * scale - lse).  An attended key has
// s * scale <= lse, so p <= 1; a masked key may score above its row's lse, and a padding key (zero K row, score 0) sits above a negative
// lse: from a gap of 88.7 on exp overflows fp32.  Zeroing such a key by a PRODUCT with 0, or relying on its zero K / V rows, then gives
// 0 * inf or inf * 0 = NaN (measured: NaN in dq / dk / dv from |q|, |k| elements of 3.5 aligned over a 64-wide head, 4.25 over 32).
// So the mask goes INTO the exponent: kvalid holds 0 for an attended key and -inf for a masked or padding one and is added in front of
// the exp2 (a v_sub_f32 for the v_mul_f32; every family works in the exp2 domain).  Without a key mask the frag kernels have no
// kvalid in their loop; there the exponent is clamped at 0 (one v_min_f32), which an attended key never exceeds by more than its
// last place, and the finite p of a padding key meets the zero K / V rows as before.
//
// What differs between the three backward families:
//   MASKED   : kvalid in the exponent (true), or the exponent clamped at 0 (false: the frag kernels without a key mask)
//   SCALE_DS : 1/sqrt(hd) applied to every dS element (true), or once to the dQ / dK accumulators in store_tile (false: frag)
//   GUARD    : score tiles at or past nt are skipped and give dS = P = 0 (true), or every tile of a block is computed (false: streamed,
//              whose padding rows carry lse = +inf / kvalid = -inf)
template <bool MASKED_, bool SCALE_DS_, bool GUARD_>
struct BwdForm {
    static constexpr bool MASKED = MASKED_, SCALE_DS = SCALE_DS_, GUARD = GUARD_;
};

// Statistics rows [0, nrows) of one sequence into LDS: lse * log2 e (exp2 domain; +inf for rows >= T), delta = rowsum(dO . O),
// kvalid (0 = key attended, -inf = masked / padding).  The general and the streamed kernel; the frag kernels take them from fragments.
template <int HG>
__device__ __forceinline__ void stats_rows(const SeqView<HG>& sv, const float* lse, int nrows, int stride, float* lse_s, float* delta,
                                           float* kvalid) {
    for (int r = threadIdx.x; r < nrows; r += stride) {
        float l = INFINITY, dl = 0.f, kv = -INFINITY;
        if (r < sv.T) {
            l = lse[sv.lse_index(r)] * LOG2E;
            kv = (sv.km && sv.km[r]) ? -INFINITY : 0.f;
#pragma unroll
            for (int c = 0; c < HG / 8; ++c) {
                const bf16x8 x = *reinterpret_cast<const bf16x8*>(sv.dO + (long)r * sv.D + c * 8);
                const bf16x8 y = *reinterpret_cast<const bf16x8*>(sv.O + (long)r * sv.D + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) dl += bf2f(x[e]) * bf2f(y[e]);
            }
        }
        lse_s[r] = l; delta[r] = dl; kvalid[r] = kv;
    }
}

__device__ __forceinline__ f32x4 splat4(float v) { return f32x4{v, v, v, v}; }

// What a tile pair does to dP under dropout of the probabilities.  NoDrop (every parent kernel): nothing, and nothing is compiled.
// DropBits (attention_stream.hip's _drop kernels): dP <- dP o m * scale, bit 4 u + r = accumulator row r of tile u of the pair is kept.
struct NoDrop {
    static constexpr bool ON = false;
};
struct DropBits {
    static constexpr bool ON = true;
    uint32_t bits;
    float scale;
    __device__ __forceinline__ void mask_dp(int u, f32x4& dp) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[r] = (bits >> (4 * u + r)) & 1u ? dp[r] * scale : 0.f;
    }
    // the bf16 probabilities of the pair as pack_tiles lays them out (element e = tile e / 4, row e % 4): P o m
    __device__ __forceinline__ bf16x8 mask_p(bf16x8 pf) const {
#pragma unroll
        for (int e = 0; e < 8; ++e) pf[e] = (bits >> e) & 1u ? pf[e] : f2bf(0.f);
        return pf;
    }
};

// S and dP of one 16 x 16 tile: image rows [t*16, t*16+16) against the wave's own-tile fragments (k = head dim).
template <int HD>
__device__ __forceinline__ void s_dp_tile(const char* img0, const char* img1, int t, const bf16x8 (&f0)[HD / 32], const bf16x8 (&f1)[HD / 32],
                                          int lane, f32x4& s, f32x4& dp) {
    s = dp = splat4(0.f);
#pragma unroll
    for (int ks = 0; ks < HD / 32; ++ks) {
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img0, t * 16, ks, lane), f0[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag<HD>(img1, t * 16, ks, lane), f1[ks], dp, 0, 0, 0);
    }
}
// p = exp(s * scale - lse) = exp2(s * (scale * log2 e) - lse * log2 e): one fma + v_exp_f32 per score; ds = p * (dp - delta).
template <class F>
__device__ __forceinline__ void p_ds_tile(f32x4 s, f32x4 dp, f32x4 kv, f32x4 lse, f32x4 delta, float scale, float scale2, f32x4& p4, f32x4& ds4) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float p;
        if constexpr (F::MASKED) p = __builtin_amdgcn_exp2f(fmaf(s[r], scale2, kv[r] - lse[r]));   // kv: 0 / -inf, see the note above
        else p = __builtin_amdgcn_exp2f(fminf(fmaf(s[r], scale2, -lse[r]), 0.f));
        p4[r] = p;
        if constexpr (F::SCALE_DS) ds4[r] = p * (dp[r] - delta[r]) * scale;
        else ds4[r] = p * (dp[r] - delta[r]);
    }
}

// Phase A, one 32-key chunk c of the K (img0) / V (img1) images against the wave's 16 queries (queries on the lane, keys on the
// accumulator rows): S^T and dP^T -> dS^T as the bf16 B operand of the dQ MFMAs.  kvalid: the image's rows.
template <int HD, class F, class DM = NoDrop>
__device__ __forceinline__ bf16x8 phase_a_pair(const char* img0, const char* img1, int c, int nt, const bf16x8 (&qf)[HD / 32],
                                               const bf16x8 (&dof)[HD / 32], const float* kvalid, float my_lse, float my_delta, float scale,
                                               float scale2, int lane, const DM& dm = DM()) {
    f32x4 ds2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int kt = 2 * c + u;
        ds2[u] = splat4(0.f);
        if (!F::GUARD || kt < nt) {
            f32x4 s, dp, p, kv = splat4(0.f);
            s_dp_tile<HD>(img0, img1, kt, qf, dof, lane, s, dp);
            if constexpr (DM::ON) dm.mask_dp(u, dp);
            if constexpr (F::MASKED) kv = *reinterpret_cast<const f32x4*>(kvalid + kt * 16 + 4 * (lane >> 4));
            p_ds_tile<F>(s, dp, kv, splat4(my_lse), splat4(my_delta), scale, scale2, p, ds2[u]);
        }
    }
    return pack_tiles(ds2[0], ds2[1]);
}
// Phase B, one 32-query chunk c of the Q (img0) / dO (img1) images against the wave's 16 keys (keys on the lane, queries on the
// accumulator rows): S and dP -> P and dS as the bf16 B operands of the dV / dK MFMAs.  lse_s, delta: the image's rows.
template <int HD, class F, class DM = NoDrop>
__device__ __forceinline__ void phase_b_pair(const char* img0, const char* img1, int c, int nt, const bf16x8 (&kf)[HD / 32],
                                             const bf16x8 (&vf)[HD / 32], const float* lse_s, const float* delta, float my_kv, float scale,
                                             float scale2, int lane, bf16x8& pf, bf16x8& dsf, const DM& dm = DM()) {
    f32x4 p2[2], ds2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int qt = 2 * c + u;
        p2[u] = ds2[u] = splat4(0.f);
        if (!F::GUARD || qt < nt) {
            f32x4 s, dp;
            s_dp_tile<HD>(img0, img1, qt, kf, vf, lane, s, dp);
            if constexpr (DM::ON) dm.mask_dp(u, dp);
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qt * 16 + 4 * (lane >> 4));
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta + qt * 16 + 4 * (lane >> 4));
            p_ds_tile<F>(s, dp, splat4(my_kv), l4, d4, scale, scale2, p2[u], ds2[u]);
        }
    }
    pf = pack_tiles(p2[0], p2[1]);
    dsf = pack_tiles(ds2[0], ds2[1]);
}

// Row `row` of a dq / dk / dv accumulator set as bf16 (SCALE_ACC: x scale first, where the family left 1/sqrt(hd) to the accumulator),
// and the running column sums of the ROUNDED values: dbias is the column sum of dqkv as stored.
template <bool SCALE_ACC>
__device__ __forceinline__ void store_row(bf16_t* dst, f32x4 acc, f32x4& cs, float scale) {
    bf16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        ov[r] = SCALE_ACC ? f2bf(acc[r] * scale) : f2bf(acc[r]);
        cs[r] += bf2f(ov[r]);
    }
    *reinterpret_cast<bf16x4*>(dst) = ov;
}
template <bool SCALE_ACC, int DT>
__device__ __forceinline__ void store_tile(bf16_t* dst, long ld, int row, int T, const f32x4 (&acc)[DT], f32x4 (&cs)[DT], int g, float scale = 1.f) {
    if (row < T) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) store_row<SCALE_ACC>(dst + (long)row * ld + dt * 16 + 4 * g, acc[dt], cs[dt], scale);
    }
}

// dbias: the column sums of dq | dk | dv (part 0 | 1 | 2) of one (sequence, head) meet in bsum and leave as this head's slice of the
// sequence's dbias_ws row (plain stores; the entry point folds the B rows afterwards: atomics from every workgroup into the same 3*D
// addresses cost 70-80 us per launch).  Default: bsum is [3*HD] and the waves meet in LDS float atomics, whose order follows wave
// timing.  DET (wj_attn_bwd_args.deterministic, a separate instantiation of the whole-image kernels; the streamed kernel in both
// modes): bsum is [NWAVES][3*HD], every wave stores its own row and the rows are added in wave order.
template <int HD, int NWAVES, bool DET>
__device__ __forceinline__ void bsum_zero(float* bsum) {
    for (int x = threadIdx.x; x < (DET ? NWAVES : 1) * 3 * HD; x += blockDim.x) bsum[x] = 0.f;
}
template <int HD, bool DET, int DT>
__device__ __forceinline__ void bsum_add(float* bsum, int part, const f32x4 (&cs)[DT], int wave, int lane) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = row16_sum(cs[dt][r]);
            if (i == 0) {
                if constexpr (DET) bsum[wave * 3 * HD + part * HD + dt * 16 + 4 * g + r] = v;
                else atomicAdd(bsum + part * HD + dt * 16 + 4 * g + r, v);
            }
        }
}
template <int HD, int HG, int NWAVES, bool DET>
__device__ __forceinline__ void dbias_store(const float* bsum, float* dbias_ws, const SeqView<HG>& sv, int stride) {
    for (int x = threadIdx.x; x < 3 * HD; x += stride) {
        const int part = x / HD, d = x - part * HD;
        float tot = bsum[x];
        if constexpr (DET) {
#pragma unroll
            for (int w = 1; w < NWAVES; ++w) tot += bsum[w * 3 * HD + x];
        }
        if (d < HG) dbias_ws[(long)sv.b * 3 * sv.D + part * sv.D + sv.h * HG + d] = tot;
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Dynamic LDS of the whole-image kernels for `rows` image rows (KP, or an instantiation's most): two padded images, then one float row
// of key-mask addends (forward) or the three statistics rows and bsum (backward).  The kernels carve smem up by the same functions.
constexpr int attn_images_bytes(int hd, int rows) { return 2 * rows * (hd * 2 + 32); }
constexpr int attn_fwd_lds_bytes(int hd, int rows) { return attn_images_bytes(hd, rows) + rows * 4; }
constexpr int attn_bwd_bsum_offset(int hd, int rows) { return attn_images_bytes(hd, rows) + 3 * rows * 4; }
constexpr int attn_bwd_lds_bytes(int hd, int rows, bool det, int waves) { return attn_bwd_bsum_offset(hd, rows) + (det ? waves : 1) * 3 * hd * 4; }

// The argument checks of the four entry points, every error answered before a launch.
struct AttnLimits {
    int t_max;      // longest sequence of the family
    int t_max16;    // longest sequence with 16-wide heads; 0: the family has no 16-wide heads
};
template <class Args>
int attn_check_dims(const Args* a, AttnLimits lim) {
    if (a->B <= 0 || a->T <= 0 || a->T > lim.t_max || a->H <= 0 || a->mask_group < 1) return WJ_ERR_ARG;
    if (a->seq_off && a->key_mask) return WJ_ERR_ARG;
    if (a->hd == 16 ? a->T > lim.t_max16 : (a->hd != 32 && a->hd != 64)) return WJ_ERR_UNSUPPORTED;
    return WJ_OK;
}
inline int attn_check_args(const wj_attn_fwd_args* a, AttnLimits lim) {
    if (!a || !a->qkv || !a->out) return WJ_ERR_ARG;
    return attn_check_dims(a, lim);
}
inline int attn_check_args(const wj_attn_bwd_args* a, AttnLimits lim) {
    if (!a || !a->qkv || !a->out || !a->dout || !a->lse || !a->dqkv) return WJ_ERR_ARG;
    const int rc = attn_check_dims(a, lim);
    if (rc != WJ_OK) return rc;
    return a->dbias && !a->dbias_ws ? WJ_ERR_ARG : WJ_OK;
}
// dbias_ws of both backward entries: one row of 3 * H * hd floats per sequence
inline int64_t attn_dbias_row(const wj_attn_bwd_args* a) { return (int64_t)3 * a->H * a->hd; }
// The tail of both backward entries: the B rows of dbias_ws into dbias, unless the caller folds them later.
inline int attn_fold_dbias(const wj_attn_bwd_args* a, void* stream) {
    if (!a->dbias || a->defer_fold) return WJ_OK;
    wj_colsum_args c = {};
    c.deterministic = a->deterministic;
    c.x = a->dbias_ws; c.out = a->dbias; c.ldx = attn_dbias_row(a); c.M = a->B; c.N = (int)attn_dbias_row(a);
    return wj_colsum_f32(&c, stream);
}

}  // namespace
