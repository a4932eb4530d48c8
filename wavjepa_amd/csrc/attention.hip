// Key-masked multi-head self-attention for short sequences (T <= 416, head dim 32/64; 16 in the 32-wide geometry) on gfx950.
//
// One workgroup (4 waves) per (batch, head).  The whole K/V (forward) or K,V then Q,dO (backward) of that head
// lives in LDS as ONE padded image per matrix ([rows][hd*2+32 bytes]) that serves both the row reads
// (ds_read_b128 -> MFMA operand with k = head dim) and the transposed reads (ds_read_b64_tr_b16 -> MFMA operand
// with k = sequence), conflict-free for both.  Scores are computed TRANSPOSED (S^T = K Q^T) so that the softmax
// reduction runs over registers + two cross-lane shuffles, and the fp32 accumulator tile is converted in place
// to the bf16 B-operand of the following MFMA (O^T = V^T P^T): P never goes through LDS.
//   forward : S^T -> mask/softmax -> O^T, LSE
//   backward: phase A (per query tile)  dQ^T = K^T dS^T        with S^T, dP^T = V dO^T recomputed
//             phase B (per key tile)    dV^T = dO^T P, dK^T = Q^T dS   with S = Q K^T, dP = dO V^T recomputed
// The operand helpers, the sequence view and the backward's tile pairs, stores and dbias epilogue are attention_pieces.h's, shared with
// attention_stream.hip; what is here is how rows reach the images (RowRegs), the walk over the tiles and the dispatch.
#include "attention_pieces.h"

namespace {

constexpr int MAX_TILES = 14;  // 16-row tiles of the default instantiation: T <= 224
constexpr int MAX_TILES_LONG = 26;  // T <= 416 (4.01 s clips -> 400 tokens): K + V images of a 64-wide head = 133 KB of LDS
constexpr int NWB64 = 4, NWB32 = 4;   // backward waves per workgroup (more waves measured slower: 339 -> 439 us at hd 64)
constexpr int NWF_LONG = 7;    // forward, T > 128: 13 query tiles over 7 waves (2,2,2,2,2,2,1) instead of 4 (4,3,3,3)
constexpr AttnLimits WHOLE_IMAGE_LIMITS = {MAX_TILES_LONG * 16, MAX_TILES * 16};   // (16-wide heads: the tiny configuration, T <= 224)
constexpr int NWF_SHORT = 4;   // forward, T <= 128 (ragged student / predictor): <= 2 tiles per wave, twice the workgroups per CU

// Copy rows [0,T) of TWO [T][ld] bf16 matrices (HD columns each) into their padded LDS images; rows [T,KP) are zero.
// All global loads of a thread are issued before its first LDS store (a load->store loop would serialise one HBM/L2
// round trip per iteration: ~13 of them for a 200 x 64 head).
template <int HD, int NWAVES, int MT = MAX_TILES, int HG = HD>
struct RowRegs {
    static constexpr int CH = Img<HD>::CH, RS = Img<HD>::RS;
    static constexpr int MAXI = (MT * 16 * CH + NWAVES * 64 - 1) / (NWAVES * 64);
    uint4 v0[MAXI], v1[MAXI];

    __device__ __forceinline__ void load(const bf16_t* __restrict__ src0, long ld0, const bf16_t* __restrict__ src1, long ld1, int T) {
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int idx = threadIdx.x + it * (NWAVES * 64);
            const int row = idx / CH, c = idx - row * CH;
            v0[it] = v1[it] = make_uint4(0, 0, 0, 0);
            if (row < T && c * 8 < HG) {     // (HG < HD: a 16-wide head in the 32-wide geometry, its upper half zeros)
                v0[it] = *reinterpret_cast<const uint4*>(src0 + (long)row * ld0 + c * 8);
                v1[it] = *reinterpret_cast<const uint4*>(src1 + (long)row * ld1 + c * 8);
            }
        }
    }
    __device__ __forceinline__ void store(char* img0, char* img1, int KP) const {
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int idx = threadIdx.x + it * (NWAVES * 64);
            const int row = idx / CH, c = idx - row * CH;
            if (row < KP) {
                *reinterpret_cast<uint4*>(img0 + row * RS + c * 16) = v0[it];
                *reinterpret_cast<uint4*>(img1 + row * RS + c * 16) = v1[it];
            }
        }
    }
};

template <int HD, int NWAVES, int MT = MAX_TILES, int HG = HD>
__device__ __forceinline__ void fill_images2(char* img0, const bf16_t* __restrict__ src0, long ld0, char* img1,
                                             const bf16_t* __restrict__ src1, long ld1, int T, int KP) {
    RowRegs<HD, NWAVES, MT, HG> r;
    r.load(src0, ld0, src1, ld1, T);
    r.store(img0, img1, KP);
}

// ------------------------------------------------------------------------------------------------ forward
// MT = most 16-row tiles a sequence may have (14: T <= 224; 8: T <= 128, fewer live registers -> more waves per SIMD)
template <int HD, int NWF, int MT, int HG = HD>
__global__ __launch_bounds__(NWF * 64, MT == 14 ? 4 : (MT == 8 ? (HD == 64 ? 4 : 6) : (MT == 12 ? 4 : 2))) void attn_fwd_kernel(wj_attn_fwd_args a) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HG / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SeqView<HG> sv(a);              // HG: the head width in memory (16 runs in the 32-wide geometry)
    const int T = sv.T, D = sv.D;
    const int nkt = (T + 15) / 16, KP = ((T + 31) / 32) * 32, nch = KP / 32;
    char* kimg = smem;
    char* vimg = smem + KP * RS;
    float* madd = reinterpret_cast<float*>(smem + attn_images_bytes(HD, KP));

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = sv.ld;
    const bf16_t* base = sv.qkv;
    bf16x8 qf[KS];                       // this wave's first query tile: in flight while K / V are staged
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = row_frag_global(base, ld, wave * 16, T, ks, lane, HG);
    fill_images2<HD, NWF, MT, HG>(kimg, base + D, ld, vimg, base + 2 * D, ld, T, KP);
    for (int k = threadIdx.x; k < KP; k += blockDim.x)
        madd[k] = (k < T && !(sv.km && sv.km[k])) ? 0.f : -INFINITY;
    __syncthreads();

    // softmax in the exp2 domain on the RAW scores: max over s, then p = exp2(s * (scale * log2 e) - max * (scale * log2 e)) -- one
    // fma + v_exp_f32 per score
    const float scale = rsqrtf((float)HG), scale2 = scale * LOG2E;
    for (int qt = wave; qt < nkt; qt += NWF) {
        bf16x8 qn[KS];                   // next tile's fragments: issued now, consumed at the end of this iteration
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qn[ks] = row_frag_global(base, ld, (qt + NWF) * 16, (qt + NWF < nkt) ? T : 0, ks, lane, HG);
        f32x4 s[MT];
        float mx = -INFINITY;
        // key tiles go in PAIRS (one 32-row chunk of the image; the second tile of the last chunk may be all padding: zero K rows
        // under a -inf mask): half the branches, and two independent MFMA chains for the scheduler to interleave
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            s[2 * c] = s[2 * c + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < nch) {
#pragma unroll
                for (int u = 0; u < 2; ++u) score_tile<HD>(s[2 * c + u], kimg, madd, 2 * c + u, qf, lane);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[2 * c + u][r]);
            }
        }
        mx = group_max(mx);
        const float msafe = (mx == -INFINITY) ? 0.f : mx;  // fully masked row: all p = 0 (the reference yields NaN)
        const float m2 = msafe * scale2;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            if (c < nch) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(s[2 * c + u][r], scale2, -m2));
                        s[2 * c + u][r] = p;
                        sum += p;
                    }
            }
        }
        sum = group_sum(sum);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            if (c < nch) {
                // probabilities are normalised BEFORE the bf16 rounding (as a materialised softmax would be)
                const bf16x8 pf = pack_tiles(s[2 * c] * inv, s[2 * c + 1] * inv);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(vimg, c, dt * 16, lane), pf, o[dt], 0, 0, 0);
            }
        }
        store_out_lse<HG>(sv, a, qt * 16 + i, o, sum, msafe, scale, g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
    }
}

// ------------------------------------------------------------------------------------------------ backward
// The LDS of both whole-image backward kernels: the two images, three statistics rows of KP floats, bsum (attn_bwd_lds_bytes).
template <int HD>
struct BwdLds {
    char *img0, *img1;               // phase A: K, V      phase B: Q, dO
    float *lse_s, *delta, *kvalid;   // [KP] each (stats_rows)
    float* bsum;                     // [3*HD], DET: [NWB][3*HD] column sums of dq | dk | dv (in_proj_bias grad)
    __device__ __forceinline__ BwdLds(char* smem, int KP) {
        img0 = smem;
        img1 = smem + KP * Img<HD>::RS;
        lse_s = reinterpret_cast<float*>(smem + attn_images_bytes(HD, KP));
        delta = lse_s + KP;
        kvalid = delta + KP;
        bsum = reinterpret_cast<float*>(smem + attn_bwd_bsum_offset(HD, KP));
    }
};

// The general kernel: any T of its instantiation, fragments of the wave's own tile prefetched one tile ahead.
template <int HD, int NWB, int MT, int HG = HD, bool DET = false>
__global__ __launch_bounds__(NWB * 64, MT > 14 ? 2 : (HD == 64 ? 3 : 4)) void attn_bwd_kernel(wj_attn_bwd_args a) {
    constexpr int KS = HD / 32, DT = HG / 16;
    using Form = BwdForm<true, true, true>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SeqView<HG> sv(a);              // HG: the head width in memory (16 runs in the 32-wide geometry)
    const int T = sv.T, D = sv.D;
    const int nt = (T + 15) / 16, KP = ((T + 31) / 32) * 32, nch = KP / 32;
    const BwdLds<HD> l(smem, KP);
    bsum_zero<HD, NWB, DET>(l.bsum);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = sv.ld;
    const bf16_t *qkv = sv.qkv, *dO = sv.dO;

    fill_images2<HD, NWB, MT, HG>(l.img0, qkv + D, ld, l.img1, qkv + 2 * D, ld, T, KP);
    // short sequences: phase B's Q / dO rows are fetched NOW (a few registers per thread) and only parked in LDS once phase A
    // is done with the K / V images -- their global latency hides behind the statistics loop and phase A
    constexpr bool EARLY = MT <= 8 && HD == 32;   // (the 64-wide head has no registers to spare at 3 waves per SIMD)
    RowRegs<HD, NWB, MT, HG> nxt;
    if constexpr (EARLY) nxt.load(qkv, ld, dO, D, T);
    stats_rows<HG>(sv, a.lse, KP, blockDim.x, l.lse_s, l.delta, l.kvalid);
    __syncthreads();
    const float scale = rsqrtf((float)HG), scale2 = scale * LOG2E;
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase A: dQ for 16 queries per wave iteration
    f32x4 csq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csq[dt] = zero4;
    bf16x8 qf[KS], dof[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = row_frag_global(qkv, ld, wave * 16, T, ks, lane, HG);
        dof[ks] = row_frag_global(dO, D, wave * 16, T, ks, lane, HG);
    }
    for (int qt = wave; qt < nt; qt += NWB) {
        bf16x8 qn[KS], don[KS];          // prefetch of the next query tile
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qn[ks] = row_frag_global(qkv, ld, (qt + NWB) * 16, (qt + NWB < nt) ? T : 0, ks, lane, HG);
            don[ks] = row_frag_global(dO, D, (qt + NWB) * 16, (qt + NWB < nt) ? T : 0, ks, lane, HG);
        }
        const float my_lse = l.lse_s[qt * 16 + i], my_delta = l.delta[qt * 16 + i];
        f32x4 dq[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] = zero4;
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            if (c < nch) {
                const bf16x8 dsf = phase_a_pair<HD, Form>(l.img0, l.img1, c, nt, qf, dof, l.kvalid, my_lse, my_delta, scale, scale2, lane);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img0, c, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
            }
        }
        store_tile<false>(sv.dqkv, ld, qt * 16 + i, T, dq, csq, g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { qf[ks] = qn[ks]; dof[ks] = don[ks]; }
    }
    if (a.dbias) bsum_add<HD, DET>(l.bsum, 0, csq, wave, lane);
    __syncthreads();
    if constexpr (EARLY) nxt.store(l.img0, l.img1, KP);
    else fill_images2<HD, NWB, MT, HG>(l.img0, qkv, ld, l.img1, dO, D, T, KP);
    __syncthreads();

    // ---- phase B: dK, dV for 16 keys per wave iteration
    f32x4 csk[DT], csv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csk[dt] = csv[dt] = zero4;
    bf16x8 kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = row_frag_global(qkv + D, ld, wave * 16, T, ks, lane, HG);
        vf[ks] = row_frag_global(qkv + 2 * D, ld, wave * 16, T, ks, lane, HG);
    }
    for (int kt = wave; kt < nt; kt += NWB) {
        bf16x8 kn[KS], vn[KS];           // prefetch of the next key tile
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kn[ks] = row_frag_global(qkv + D, ld, (kt + NWB) * 16, (kt + NWB < nt) ? T : 0, ks, lane, HG);
            vn[ks] = row_frag_global(qkv + 2 * D, ld, (kt + NWB) * 16, (kt + NWB < nt) ? T : 0, ks, lane, HG);
        }
        const float my_kv = l.kvalid[kt * 16 + i];
        f32x4 dk[DT], dv[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = zero4;
#pragma unroll
        for (int c = 0; c < MT / 2; ++c) {
            if (c < nch) {
                bf16x8 pf, dsf;
                phase_b_pair<HD, Form>(l.img0, l.img1, c, nt, kf, vf, l.lse_s, l.delta, my_kv, scale, scale2, lane, pf, dsf);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img1, c, dt * 16, lane), pf, dv[dt], 0, 0, 0);
                    dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img0, c, dt * 16, lane), dsf, dk[dt], 0, 0, 0);
                }
            }
        }
        store_tile<false>(sv.dqkv + D, ld, kt * 16 + i, T, dk, csk, g);
        store_tile<false>(sv.dqkv + 2 * D, ld, kt * 16 + i, T, dv, csv, g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) { kf[ks] = kn[ks]; vf[ks] = vn[ks]; }
    }
    if (a.dbias) {
        bsum_add<HD, DET>(l.bsum, 1, csk, wave, lane);
        bsum_add<HD, DET>(l.bsum, 2, csv, wave, lane);
        __syncthreads();
        dbias_store<HD, HG, NWB, DET>(l.bsum, a.dbias_ws, sv, blockDim.x);
    }
}

// hipcc leaves the VALU read of an MFMA result one wait state short when the MFMA sits right in front of a loop's exit branch and the
// read behind it (tools/mfma_hazard_scan.py).  The frag kernels' 16-wide heads have one output tile per accumulator set, so the last
// MFMA of the chunk loop is in exactly that place: eight wait states by hand.
template <bool ON>
__device__ __forceinline__ void mfma_exit_wait() {
    if constexpr (ON) asm volatile("s_nop 7" ::: "memory");
}

// Backward for SHORT sequences (T <= 128: ragged student / predictor), one global round trip per workgroup.
// The general kernel above walks four dependent fetches (K/V images -> statistics rows -> Q/dO fragments -> K/V fragments again),
// each a full HBM/L2 latency with only 4 workgroups per CU to hide it (stamps: a predictor workgroup lives ~20 us for ~2 us of
// issue).  Here every wave fetches, at entry, the MFMA row fragments of ITS OWN <= 2 tiles of K, V, Q, dO and O (lane (i,g) = row i,
// 16-B chunk g: exactly the B-operand layout) plus lse / key mask for those rows, and everything downstream is fed from them:
//   * the K / V fragments are written to the LDS images for phase A and stay in registers as phase B's own-tile operands,
//   * the Q / dO fragments are phase A's own-tile operands and are written to the images once phase A is done,
//   * delta = rowsum(dO . O) falls out of the dO / O fragments with two cross-lane adds.
// The 1/sqrt(hd) of dS is applied once to the dQ / dK accumulators (as the flash kernels do) instead of to every dS element.
// Without a key mask nothing needs masking at all: K / V rows >= T are zero in the images, so a padding key adds 0 to dQ, and the
// dK / dV rows of padding keys are never stored; padding QUERIES have lse = +inf, p = 0.
template <int HD, int NWB, int MT, bool MASKED, int HG = HD, bool DET = false>
__global__ __launch_bounds__(NWB * 64, HD == 64 ? 3 : 4) void attn_bwd_frag_kernel(wj_attn_bwd_args a) {
    constexpr int RS = Img<HD>::RS, KS = HD / 32, DT = HG / 16, TPW = MT / NWB;
    static_assert(MT % NWB == 0, "tiles are dealt to waves round-robin");
    using Form = BwdForm<MASKED, false, true>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const SeqView<HG> sv(a);              // HG: the head width in memory (16 runs in the 32-wide geometry)
    const int T = sv.T, D = sv.D;
    const int nt = (T + 15) / 16, KP = ((T + 31) / 32) * 32, nch = KP / 32;
    const BwdLds<HD> l(smem, KP);
    bsum_zero<HD, NWB, DET>(l.bsum);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const long ld = sv.ld;
    const bf16_t *qkv = sv.qkv, *dO = sv.dO;

    bf16x8 kfr[TPW][KS], vfr[TPW][KS], qfr[TPW][KS], dofr[TPW][KS];
    float lse_r[TPW], delta_r[TPW], kv_r[TPW];
    {
        bf16x8 ofr[TPW][KS];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {          // every fetch of the workgroup's life, back to back
            const int rb = (wave + t * NWB) * 16, row = rb + i;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                kfr[t][ks] = row_frag_global(qkv + D, ld, rb, T, ks, lane, HG);
                vfr[t][ks] = row_frag_global(qkv + 2 * D, ld, rb, T, ks, lane, HG);
                qfr[t][ks] = row_frag_global(qkv, ld, rb, T, ks, lane, HG);
                dofr[t][ks] = row_frag_global(dO, D, rb, T, ks, lane, HG);
                ofr[t][ks] = row_frag_global(sv.O, D, rb, T, ks, lane, HG);
            }
            lse_r[t] = INFINITY; kv_r[t] = -INFINITY;
            if (row < T) {
                lse_r[t] = a.lse[sv.lse_index(row)] * LOG2E;
                kv_r[t] = (sv.km && sv.km[row]) ? -INFINITY : 0.f;
            }
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int rb = (wave + t * NWB) * 16, row = rb + i;
            float dl = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) dl += bf2f(dofr[t][ks][e]) * bf2f(ofr[t][ks][e]);
            delta_r[t] = group_sum(dl);
            if (rb < KP) {                        // rows [T, KP) carry zeros / +inf (fragments of rows >= T are zero)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    *reinterpret_cast<bf16x8*>(l.img0 + row * RS + (ks * 4 + g) * 16) = kfr[t][ks];
                    *reinterpret_cast<bf16x8*>(l.img1 + row * RS + (ks * 4 + g) * 16) = vfr[t][ks];
                }
                if (g == 0) { l.lse_s[row] = lse_r[t]; l.delta[row] = delta_r[t]; l.kvalid[row] = kv_r[t]; }
            }
        }
    }
    __syncthreads();
    const float scale = rsqrtf((float)HG), scale2 = scale * LOG2E;
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase A: dQ of this wave's query tiles
    f32x4 csq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csq[dt] = zero4;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int qt = wave + t * NWB;
        if (qt < nt) {
            f32x4 dq[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dq[dt] = zero4;
#pragma unroll
            for (int c = 0; c < MT / 2; ++c) {
                if (c < nch) {
                    const bf16x8 dsf = phase_a_pair<HD, Form>(l.img0, l.img1, c, nt, qfr[t], dofr[t], l.kvalid, lse_r[t], delta_r[t], scale, scale2, lane);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
                        dq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img0, c, dt * 16, lane), dsf, dq[dt], 0, 0, 0);
                }
            }
            mfma_exit_wait<(HG < HD)>();
            store_tile<true>(sv.dqkv, ld, qt * 16 + i, T, dq, csq, g, scale);
        }
    }
    if (a.dbias) bsum_add<HD, DET>(l.bsum, 0, csq, wave, lane);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int rb = (wave + t * NWB) * 16, row = rb + i;
        if (rb < KP) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                *reinterpret_cast<bf16x8*>(l.img0 + row * RS + (ks * 4 + g) * 16) = qfr[t][ks];
                *reinterpret_cast<bf16x8*>(l.img1 + row * RS + (ks * 4 + g) * 16) = dofr[t][ks];
            }
        }
    }
    __syncthreads();

    // ---- phase B: dK, dV of this wave's key tiles
    f32x4 csk[DT], csv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) csk[dt] = csv[dt] = zero4;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int kt = wave + t * NWB;
        if (kt < nt) {
            f32x4 dk[DT], dv[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = zero4;
#pragma unroll
            for (int c = 0; c < MT / 2; ++c) {
                if (c < nch) {
                    bf16x8 pf, dsf;
                    phase_b_pair<HD, Form>(l.img0, l.img1, c, nt, kfr[t], vfr[t], l.lse_s, l.delta, kv_r[t], scale, scale2, lane, pf, dsf);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img1, c, dt * 16, lane), pf, dv[dt], 0, 0, 0);
                        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag<HD>(l.img0, c, dt * 16, lane), dsf, dk[dt], 0, 0, 0);
                    }
                }
            }
            mfma_exit_wait<(HG < HD)>();
            store_tile<true>(sv.dqkv + D, ld, kt * 16 + i, T, dk, csk, g, scale);
            store_tile<false>(sv.dqkv + 2 * D, ld, kt * 16 + i, T, dv, csv, g);
        }
    }
    if (a.dbias) {
        bsum_add<HD, DET>(l.bsum, 1, csk, wave, lane);
        bsum_add<HD, DET>(l.bsum, 2, csv, wave, lane);
        __syncthreads();
        dbias_store<HD, HG, NWB, DET>(l.bsum, a.dbias_ws, sv, blockDim.x);
    }
}

template <typename K>
int set_lds(K kern, int bytes) {
    return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 0 : -1;
}

// The backward dispatch, written once for both modes: DET = true launches the deterministic twin of every branch (per-wave bsum rows:
// NW - 1 more rows of LDS).
template <bool DET>
void launch_bwd(const wj_attn_bwd_args* a, hipStream_t st) {
    const int hdk = a->hd == 16 ? 32 : a->hd;
    const int KP = ((a->T + 31) / 32) * 32;
    const int lds = attn_bwd_lds_bytes(hdk, KP, DET, NWB64);
    static_assert(NWB64 == NWB32, "one wave count in lds");
    dim3 grid(a->B * a->H);
    static int once = set_lds(attn_bwd_kernel<64, NWB64, 14, 64, DET>, attn_bwd_lds_bytes(64, 14 * 16, DET, NWB64)) |
                      set_lds(attn_bwd_kernel<32, NWB32, 14, 32, DET>, attn_bwd_lds_bytes(32, 14 * 16, DET, NWB32)) |
                      set_lds(attn_bwd_kernel<64, NWB64, 26, 64, DET>, attn_bwd_lds_bytes(64, 26 * 16, DET, NWB64)) |
                      set_lds(attn_bwd_kernel<32, NWB32, 26, 32, DET>, attn_bwd_lds_bytes(32, 26 * 16, DET, NWB32));
    (void)once;
    if (a->hd == 16) {
        if (a->T <= 128) {
            if (a->key_mask) hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 8, true, 16, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
            else hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 8, false, 16, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
        } else if (a->T <= 192) {
            if (a->key_mask) hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 12, true, 16, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
            else hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 12, false, 16, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
        } else {
            hipLaunchKernelGGL((attn_bwd_kernel<32, NWB32, 14, 16, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
        }
    } else if (a->T > MAX_TILES * 16) {     // 225 .. 416 tokens
        if (a->hd == 64) hipLaunchKernelGGL((attn_bwd_kernel<64, NWB64, 26, 64, DET>), grid, dim3(NWB64 * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_bwd_kernel<32, NWB32, 26, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
    } else if (a->T <= 128) {          // ragged student / predictor: at most 8 tiles (6 or 8 waves per workgroup measured 1.5-2x slower)
        static const int frag = wj_lab_env_int("WJ_ATTN_BWD_FRAG", 3);   // bit 0: hd 32, bit 1: hd 64 (A/B switch)
        const bool masked = a->key_mask != nullptr;
        if (a->hd == 64) {
            if (!(frag & 2)) hipLaunchKernelGGL((attn_bwd_kernel<64, NWB64, 8, 64, DET>), grid, dim3(NWB64 * 64), lds, st, *a);
            else if (masked) hipLaunchKernelGGL((attn_bwd_frag_kernel<64, NWB64, 8, true, 64, DET>), grid, dim3(NWB64 * 64), lds, st, *a);
            else hipLaunchKernelGGL((attn_bwd_frag_kernel<64, NWB64, 8, false, 64, DET>), grid, dim3(NWB64 * 64), lds, st, *a);
        } else {
            if (!(frag & 1)) hipLaunchKernelGGL((attn_bwd_kernel<32, NWB32, 8, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
            else if (masked) hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 8, true, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
            else hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 8, false, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
        }
    } else if (a->hd == 64) {
        hipLaunchKernelGGL((attn_bwd_kernel<64, NWB64, 14, 64, DET>), grid, dim3(NWB64 * 64), lds, st, *a);
    } else if (a->T <= 192) {          // 129 .. 192 tokens, head dim 32: the single-round-trip kernel with three tiles per wave
        if (a->key_mask) hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 12, true, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_bwd_frag_kernel<32, NWB32, 12, false, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
    } else {
        hipLaunchKernelGGL((attn_bwd_kernel<32, NWB32, 14, 32, DET>), grid, dim3(NWB32 * 64), lds, st, *a);
    }
}

}  // namespace

extern "C" int wj_attn_fwd(const wj_attn_fwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    const int rc = attn_check_args(a, WHOLE_IMAGE_LIMITS);
    if (rc != WJ_OK) return rc;
    const int hdk = a->hd == 16 ? 32 : a->hd;             // a 16-wide head runs in the 32-wide geometry, the upper half of its K dimension zeros
    const int KP = ((a->T + 31) / 32) * 32;
    const int lds = attn_fwd_lds_bytes(hdk, KP);
    dim3 grid(a->B * a->H);
    hipStream_t st = (hipStream_t)stream;
    static int once = set_lds(attn_fwd_kernel<64, NWF_LONG, 14>, attn_fwd_lds_bytes(64, 14 * 16)) | set_lds(attn_fwd_kernel<32, NWF_LONG, 14>, attn_fwd_lds_bytes(32, 14 * 16)) |
                      set_lds(attn_fwd_kernel<64, NWF_SHORT, 8>, attn_fwd_lds_bytes(64, 8 * 16)) | set_lds(attn_fwd_kernel<32, NWF_SHORT, 8>, attn_fwd_lds_bytes(32, 8 * 16)) |
                      set_lds(attn_fwd_kernel<64, NWF_LONG, 26>, attn_fwd_lds_bytes(64, 26 * 16)) | set_lds(attn_fwd_kernel<32, NWF_LONG, 26>, attn_fwd_lds_bytes(32, 26 * 16));
    (void)once;
    const bool shortseq = a->T <= 128;
    if (a->hd == 16) {
        if (shortseq) hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_SHORT, 8, 16>), grid, dim3(NWF_SHORT * 64), lds, st, *a);
        else if (a->T <= 192) hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_SHORT, 12, 16>), grid, dim3(NWF_SHORT * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_LONG, 14, 16>), grid, dim3(NWF_LONG * 64), lds, st, *a);
    } else if (a->T > MAX_TILES * 16) {     // 225 .. 416 tokens
        if (a->hd == 64) hipLaunchKernelGGL((attn_fwd_kernel<64, NWF_LONG, 26>), grid, dim3(NWF_LONG * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_LONG, 26>), grid, dim3(NWF_LONG * 64), lds, st, *a);
    } else if (a->hd == 64) {
        if (shortseq) hipLaunchKernelGGL((attn_fwd_kernel<64, NWF_SHORT, 8>), grid, dim3(NWF_SHORT * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_fwd_kernel<64, NWF_LONG, 14>), grid, dim3(NWF_LONG * 64), lds, st, *a);
    } else {
        // 129 .. 192 tokens at head dim 32: the predictor's longest ragged sequences of a step now and then (one step in eight at the
        // AudioSet mask parameters) -- three tiles per wave in the short-sequence kernel instead of the general one (105 -> ~75 us)
        if (shortseq) hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_SHORT, 8>), grid, dim3(NWF_SHORT * 64), lds, st, *a);
        else if (a->T <= 192) hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_SHORT, 12>), grid, dim3(NWF_SHORT * 64), lds, st, *a);
        else hipLaunchKernelGGL((attn_fwd_kernel<32, NWF_LONG, 14>), grid, dim3(NWF_LONG * 64), lds, st, *a);
    }
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

// scratch of wj_attn_bwd and wj_attn_stream_bwd: the dbias_ws rows attn_fold_dbias folds
int64_t wj_attn_bwd_ws_bytes(const wj_attn_bwd_args* a) { return a->B * attn_dbias_row(a) * 4; }

extern "C" int wj_attn_bwd(const wj_attn_bwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    int rc = attn_check_args(a, WHOLE_IMAGE_LIMITS);
    if (rc != WJ_OK) return rc;
    if (a->deterministic) launch_bwd<true>(a, (hipStream_t)stream);
    else launch_bwd<false>(a, (hipStream_t)stream);
    rc = attn_fold_dbias(a, stream);
    if (rc != WJ_OK) return rc;
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
