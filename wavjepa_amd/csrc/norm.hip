// LayerNorm forward/backward (fp32 statistics, fused residual add, post- and pre-norm) and column sums for gfx950.
// HBM-bound kernels: one 64-lane wave owns a row, 16-B (fp32) / 8-B (bf16) vector accesses, wave-shuffle
// reductions; column (parameter-gradient) partials are combined in LDS before one global atomic per column per
// workgroup.  Every piece of arithmetic below exists once; the kernels differ in which operands they read and write.
#include "common.h"
#include "../../include/wavjepa_hip.h"
#include "dropout_host.h"

namespace {

constexpr int MAXV = 4;  // float4 chunks per 64-lane row: D <= 1024

// token row m -> row of a padded (seg rows per clip, `valid` of them tokens) conv buffer; chan = S > 1: the buffer is
// channel-major (clip index c*nclips + n) while token m = (n*S + c)*valid + t
__device__ __forceinline__ long remap_row(int m, int seg, int valid, int chan = 1, int nclips = 0) {
    if (seg <= 0) return (long)m;
    const int q = m / valid, t = m - q * valid;
    if (chan <= 1) return (long)q * seg + t;
    const int n = q / chan, c = q - n * chan;
    return ((long)c * nclips + n) * seg + t;
}

__device__ __forceinline__ f32x4 load4(const void* base, long row, int D, int col, bool is_bf16) {
    if (is_bf16) {
        const bf16x4 v = *reinterpret_cast<const bf16x4*>((const bf16_t*)base + row * D + col);
        return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
    }
    return *reinterpret_cast<const f32x4*>((const float*)base + row * D + col);
}

// x (f32 or bf16, row xr) + the optional bf16 addend r (row m): the row that is normalised
__device__ __forceinline__ f32x4 load4_sum(const void* x, long xr, bool x_is_bf16, const void* r, long m, int D, int col) {
    f32x4 s = load4(x, xr, D, col, x_is_bf16);
    if (r) s += load4(r, m, D, col, true);
    return s;
}

// the four keep bits of chunk (m, col) of a [M][D] tensor under dropout: group m * D / 8 + col / 8, draws col % 8 .. + 3 (the two
// chunks of a group are held by neighbouring lanes, each of which runs the generator: 60 VALU operations against a 16-byte row access)
__device__ __forceinline__ uint32_t drop_bits4(const DropParams& d, long m, int D, int col) {
    return (drop_keep_bits(d, (uint64_t)(m * (D >> 3) + (col >> 3))) >> (col & 4)) & 15u;
}
// v o m * scale
__device__ __forceinline__ f32x4 drop4(f32x4 v, uint32_t keep, float scale) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (keep >> e) & 1u ? v[e] * scale : 0.f;
    return v;
}
// x (f32 or bf16, row xr) + the bf16 addend r (row m) under dropout
__device__ __forceinline__ f32x4 load4_sum_drop(const void* x, long xr, bool x_is_bf16, const void* r, long m, int D, int col, const DropParams& d) {
    return load4(x, xr, D, col, x_is_bf16) + drop4(load4(r, m, D, col, true), drop_bits4(d, m, D, col), d.scale);
}

__device__ __forceinline__ bf16x4 round4(f32x4 v) { return bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])}; }

// a chunk in f32 (row rf of pf) and rounded to bf16 (row rb of pb), each optional
__device__ __forceinline__ void store4(float* pf, long rf, void* pb, long rb, int D, int col, f32x4 v, bf16x4 vb) {
    if (pf) *reinterpret_cast<f32x4*>(pf + rf * D + col) = v;
    if (pb) *reinterpret_cast<bf16x4*>((bf16_t*)pb + rb * D + col) = vb;
}

// LPR lanes own a row (64, or 32 when D is an odd multiple of 128 -- D = 384 would leave a quarter of a 64-lane row idle),
// V float4 chunks per lane: D <= 4 V LPR.  A wave works on 64 / LPR rows at once.  Lane li of sub-row sr holds columns
// col(j) .. col(j) + 3 of chunk j.
// The chunk walk: `LN_FOR_CHUNKS(L, j, col) { ... }` runs the block for every chunk j of the lane that lies inside the row, col its first
// column.  A loop statement, not a function taking a lambda: the same walk through a closure costs every kernel here 4-8 V registers
// (hipcc 7: row addresses are then kept per chunk instead of per row).  The macro ends in an `if` without an `else`: an `else` written
// behind its block would bind to that hidden `if` (chunks outside the row), so give the block braces and never follow it with one.
#define LN_FOR_CHUNKS(L, j, col) \
    _Pragma("unroll") for (int j = 0; j < (L).V; ++j) \
        if (const int col = (L).col(j); col < (L).D)
template <int V_, int LPR>
struct Lanes {
    static constexpr int V = V_;
    static constexpr int RPW = 64 / LPR;            // rows per wave
    static constexpr int CW = LPR * 4 * V;          // columns covered (>= D)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & (LPR - 1), sr = lane / LPR;   // LPR is 32 or 64; the mask keeps col() visibly non-negative
    const int D;
    const float invD;
    __device__ __forceinline__ explicit Lanes(int D_) : D(D_), invD(1.0f / (float)D_) {}
    __device__ __forceinline__ int col(int j) const { return li * 4 + LPR * 4 * j; }
    // chunks outside the row are never read, but start defined: left undefined they cost the forward kernels 4-16 registers
    __device__ __forceinline__ static void zero(f32x4 (&v)[V]) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // a [D] vector (gamma, beta) held in registers across the row loop
    __device__ __forceinline__ void load_vector(const float* p, f32x4 (&v)[V]) const {
        zero(v);
        LN_FOR_CHUNKS(*this, j, col) { v[j] = *reinterpret_cast<const f32x4*>(p + col); }
    }
};

template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int GS_SPLIT = WJ_GROUP_STATS_SPLIT;   // workgroups per row group when group_stats is requested

// Forward row assignment.  Default: rows interleaved over the grid.  Grouped (group_stats): a workgroup owns a contiguous quarter of
// ONE group of rows, keeps its two sums in registers and STORES the pair at the end (store_group_stats); the consumer adds the
// quarters in order (no float atomics: the teacher targets are bit-reproducible).
struct RowRange { int begin, end; unsigned step; };   // unsigned step, as the grid arithmetic it comes from: with a signed one the lean
                                                      // kernels take 6-8 more V registers (row addresses become per-chunk induction variables)
template <int V, int LPR>
__device__ __forceinline__ RowRange fwd_rows(const Lanes<V, LPR>& L, int M, bool grouped, int group_rows) {
    constexpr int RPW = Lanes<V, LPR>::RPW;
    if (!grouped) return {(int)((blockIdx.x * 4 + L.wave) * RPW + L.sr), M, gridDim.x * 4 * RPW};
    const int grp = blockIdx.x / GS_SPLIT, part = blockIdx.x - grp * GS_SPLIT;
    const int rpp = (group_rows + GS_SPLIT - 1) / GS_SPLIT;
    return {grp * group_rows + part * rpp + L.wave * RPW + L.sr, min(M, grp * group_rows + min(group_rows, (part + 1) * rpp)), 4u * RPW};
}
// A lane's running group sums take a row's share (its <= 16 elements, summed on their own) in ONE addition each.  Added element by
// element instead, a lane's sums are one chain over all its rows -- 600 elements at 200 x 768 -- and on a sample whose elements are all
// equal every addition of that chain rounds the same way: the sums came out 19 u (sum |s|) off, 2.4 x the 8 u that
// tests/norm_reference.py allows a sum (4.6 x at D = 1024); by rows they stay within 0.4 x.
__device__ __forceinline__ void add_row_to_group(float& gs1, float& gs2, float r1, float r2) {
    gs1 += r1;
    gs2 += r2;
}
// kernel-uniform call: fold lanes, then waves, then one pair of stores per workgroup into [group][GS_SPLIT][2]
__device__ __forceinline__ void store_group_stats(float* group_stats, float gs1, float gs2) {
    __shared__ float gred[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    gs1 = wave_sum(gs1);
    gs2 = wave_sum(gs2);
    if (lane == 0) { gred[wave][0] = gs1; gred[wave][1] = gs2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float* gsp = group_stats + (long)blockIdx.x * 2;
        gsp[threadIdx.x] = gred[0][threadIdx.x] + gred[1][threadIdx.x] + gred[2][threadIdx.x] + gred[3][threadIdx.x];
    }
}

// Row statistics from the lane's chunks s and their sum (accumulated by the caller's own load loop): mean, then the squared
// deviations, then rstd; stored to mean_out / rstd_out [m] where given.
template <int V, int LPR>
__device__ __forceinline__ void row_stats(const Lanes<V, LPR>& L, const f32x4 (&s)[V], float sum, float eps, float* mean_out, float* rstd_out,
                                          int m, float& mean, float& rstd) {
    mean = row_sum<LPR>(sum) * L.invD;
    float sq = 0.f;
    const float mu = mean;
    LN_FOR_CHUNKS(L, j, col) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = s[j][e] - mu;
            sq += d * d;
        }
    }
    const float var = row_sum<LPR>(sq) * L.invD;
    rstd = rsqrtf(var + eps);
    if (L.li == 0) {
        if (mean_out) mean_out[m] = mean;
        if (rstd_out) rstd_out[m] = rstd;
    }
}

__device__ __forceinline__ f32x4 normalise4(f32x4 s, float mean, float rstd, f32x4 gam, f32x4 bet) {
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (s[e] - mean) * rstd * gam[e] + bet[e];
    return y;
}

// DROP: the addend r goes through dropout (wj_layernorm_fwd_drop; no fp8 output there)
template <int V, int LPR, bool DROP>
__device__ __forceinline__ void ln_fwd_body(const wj_ln_fwd_args& a, const DropParams& d) {
    const Lanes<V, LPR> L(a.D);
    const int D = a.D;
    f32x4 gam[V], bet[V];
    L.load_vector(a.gamma, gam);
    L.load_vector(a.beta, bet);
    const RowRange rows = fwd_rows(L, a.M, a.group_stats != nullptr, a.group_rows);
    float gs1 = 0.f, gs2 = 0.f;
    for (int m = rows.begin; m < rows.end; m += rows.step) {
        const long xr = remap_row(m, a.in_seg, a.in_valid, a.in_chan, a.in_chan > 1 ? a.M / (a.in_chan * a.in_valid) : 0);
        f32x4 s[V];
        float sum = 0.f;
        L.zero(s);
        LN_FOR_CHUNKS(L, j, col) {
            if constexpr (DROP) s[j] = load4_sum_drop(a.x, xr, a.x_is_bf16, a.r, m, D, col, d);
            else s[j] = load4_sum(a.x, xr, a.x_is_bf16, a.r, m, D, col);
            sum += s[j][0] + s[j][1] + s[j][2] + s[j][3];
        }
        float mean, rstd;
        row_stats(L, s, sum, a.eps, a.mean, a.rstd, m, mean, rstd);
        float r1 = 0.f, r2 = 0.f;      // the row's share of the group sums (add_row_to_group)
        LN_FOR_CHUNKS(L, j, col) {
            const f32x4 y = normalise4(s[j], mean, rstd, gam[j], bet[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r1 += y[e];
                r2 = fmaf(y[e], y[e], r2);
            }
            const bf16x4 o = round4(y);
            store4(a.y_f32, m, a.y_bf16, m, D, col, y, o);
            if (!DROP && a.y_fp8) {
                // MX fp8 of bf16(y), as wj_quantize_mxfp8 defines it: a 32-column block = 8 consecutive lanes of this chunk, the
                // four block scales of a 128-column K tile = 32 lanes -> one dword [kt][row] (D % 128 == 0: every lane of a
                // block / K tile is live together, so the shuffles below are uniform)
                float f[4], amax = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) { f[e] = bf2f(o[e]); amax = fmaxf(amax, fabsf(f[e])); }
                amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
                amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
                amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
                int sc = 0;
                if (amax > 0.f) {
                    int ex;
                    const float mm = frexpf(amax * (1.0f / 448.0f), &ex);
                    sc = (mm == 0.5f) ? ex - 1 : ex;
                    sc = max(-127, min(127, sc));
                }
                const float inv = __builtin_amdgcn_ldexpf(1.0f, -sc);
                unsigned w = 0;
                w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, w, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, w, true);
                *reinterpret_cast<unsigned*>((unsigned char*)a.y_fp8 + (long)m * D + col) = w;
                const unsigned sb = (unsigned)(sc + 127);
                const int base = L.lane & ~31;
                const unsigned s0 = __shfl(sb, base, 64), s1 = __shfl(sb, base + 8, 64), s2 = __shfl(sb, base + 16, 64),
                               s3 = __shfl(sb, base + 24, 64);
                if ((L.lane & 31) == 0)
                    ((uint32_t*)a.y_fp8_scales)[(long)(col / 128) * a.ld_fp8_scale + m] = s0 | (s1 << 8) | (s2 << 16) | (s3 << 24);
            }
        }
        add_row_to_group(gs1, gs2, r1, r2);
    }
    if (a.group_stats) store_group_stats(a.group_stats, gs1, gs2);
}
template <int V, int LPR>
__global__ __launch_bounds__(256) void ln_fwd_kernel(wj_ln_fwd_args a) {
    ln_fwd_body<V, LPR, false>(a, DropParams{});
}
template <int V, int LPR>
__global__ __launch_bounds__(256) void ln_fwd_drop_kernel(wj_ln_fwd_args a, DropParams d) {
    ln_fwd_body<V, LPR, true>(a, d);
}

// The LEAN form (wj_ln_fwd_args.workgroups > 0): the same pieces in the same order -- bit-identical outputs -- from a kernel that fits
// beside a persistent GEMM workgroup of ANOTHER stream on the same CU.  Such a workgroup (csrc/gemm_persist.hip) holds 2 x 224-232 of a
// SIMD's 512 VGPRs and 150 of the CU's 160 KB of LDS for the whole launch: what is left is one wave of <= 48 registers per SIMD and a few
// KB of LDS.  ln_fwd_kernel (51-100 VGPRs) therefore never runs beside it: the forward's LayerNorms -- HBM-bound, matrix pipe idle -- and
// the other stream's GEMMs -- matrix-bound, HBM mostly idle -- take turns on the chip.  This form keeps gamma / beta in memory (3 KB,
// L1-resident; re-read per row), has no fp8 / group-statistics / row-remap paths, and is launched with a grid capped by the caller (one
// workgroup per CU = one wave per SIMD): it takes the bandwidth the GEMM leaves idle and never the CU slots the next persistent launch needs.
template <int V, int LPR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void ln_fwd_lean_kernel(wj_ln_fwd_args a) {
    const Lanes<V, LPR> L(a.D);
    const int D = a.D;
    const RowRange rows = fwd_rows(L, a.M, false, 0);
    for (int m = rows.begin; m < rows.end; m += rows.step) {
        f32x4 s[V];
        float sum = 0.f;
        L.zero(s);
        LN_FOR_CHUNKS(L, j, col) {
            s[j] = load4_sum(a.x, m, a.x_is_bf16, a.r, m, D, col);
            sum += s[j][0] + s[j][1] + s[j][2] + s[j][3];
        }
        float mean, rstd;
        row_stats(L, s, sum, a.eps, a.mean, a.rstd, m, mean, rstd);
        LN_FOR_CHUNKS(L, j, col) {
            const f32x4 gam = *reinterpret_cast<const f32x4*>(a.gamma + col);
            const f32x4 bet = *reinterpret_cast<const f32x4*>(a.beta + col);
            const f32x4 y = normalise4(s[j], mean, rstd, gam, bet);
            store4(a.y_f32, m, a.y_bf16, m, D, col, y, round4(y));
        }
    }
}

// ---- pre-norm (norm_first) stacks: x = x + branch(LN(x)) --------------------------------------------------------------------------
// The fusion point sits half a layer later than in the post-norm kernel above: ONE kernel adds the previous branch into the residual
// stream and normalises the sum for the next branch.  s = x (+ r) is the new stream (stored as f32, in place when s_f32 == x: a lane
// reads exactly the elements it writes), y = LN(s) the next GEMM's A operand.  group_stats are taken over s (a pre-norm layer's OUTPUT
// is the stream).  Without any of y / mean / rstd the kernel only adds (the teacher's last layer has no norm behind it).
template <int V, int LPR>
__global__ __launch_bounds__(256) void ln_pre_fwd_kernel(wj_ln_pre_fwd_args a) {
    const Lanes<V, LPR> L(a.D);
    const int D = a.D;
    const bool norm = a.y_f32 || a.y_bf16 || a.mean || a.rstd;          // kernel-uniform
    f32x4 gam[V], bet[V];
    L.load_vector(a.gamma, gam);
    L.load_vector(a.beta, bet);
    const RowRange rows = fwd_rows(L, a.M, a.group_stats != nullptr, a.group_rows);
    float gs1 = 0.f, gs2 = 0.f;
    // a signed step here: advanced by the unsigned one this kernel is scheduled into 6-10 fewer registers (V >= 2) and the short
    // launches get slower (tools/ln_bench.py, 10045 x 768: 25.4 us against 24.2; all five shapes in profiles/norm_shared_pieces.txt)
    for (int m = rows.begin; m < rows.end; m += (int)rows.step) {
        f32x4 s[V];
        float sum = 0.f, r2 = 0.f;
        L.zero(s);
        LN_FOR_CHUNKS(L, j, col) {
            s[j] = load4_sum(a.x, m, false, a.r, m, D, col);
            if (a.s_f32) *reinterpret_cast<f32x4*>(a.s_f32 + (long)m * D + col) = s[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sum += s[j][e];
                r2 = fmaf(s[j][e], s[j][e], r2);
            }
        }
        add_row_to_group(gs1, gs2, sum, r2);
        if (!norm) continue;
        float mean, rstd;
        row_stats(L, s, sum, a.eps, a.mean, a.rstd, m, mean, rstd);
        LN_FOR_CHUNKS(L, j, col) {
            const f32x4 y = normalise4(s[j], mean, rstd, gam[j], bet[j]);
            store4(a.y_f32, m, a.y_bf16, m, D, col, y, round4(y));
        }
    }
    if (a.group_stats) store_group_stats(a.group_stats, gs1, gs2);
}

constexpr int BWD_THREADS = 256;

// The backward of both norm orders.  LPR lanes per row, TWO row slots in flight per wave (independent load streams ahead of the shuffle
// reductions), V float4 chunks per lane.  Column partials (dgamma, dbeta, dbias) stay in registers across the row loop and are combined
// through LDS in wave order, then one global atomic per column per workgroup (or a workspace row, folded afterwards).
// `ops` says what the norm order decides: where a row slot's (x-hat source, dy) come from, which row of ds_bf16 a token row goes to, and
// whether a residual-path gradient is added to ds.  It exposes the entry's argument struct as `a`; M, D, gamma, mean, rstd, ds_f32,
// ds_bf16, workspace, dgamma, dbeta and dbias carry the same names in both.
template <int V, int LPR, class Ops>
__device__ __forceinline__ void ln_bwd_body(const Ops& ops) {
    const auto& a = ops.a;
    constexpr int nw = BWD_THREADS / 64;
    __shared__ float cacc[nw][3][Lanes<V, LPR>::CW];   // per-wave column partials, added in wave order below
    const Lanes<V, LPR> L(a.D);
    const int D = a.D;

    f32x4 dg[V], db[V], dbi[V], gam[V];
    L.zero(dg);
    L.zero(db);
    L.zero(dbi);
    L.load_vector(a.gamma, gam);
    const int stride = gridDim.x * nw * L.RPW;
    for (int m0 = (blockIdx.x * nw + L.wave) * L.RPW + L.sr; m0 < a.M; m0 += 2 * stride) {
        int mrow[2] = {m0, m0 + stride};
        f32x4 xh[2][V], dy[2][V];
        float mean[2], rstd[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = mrow[u] < a.M ? mrow[u] : m0;      // a dead second slot re-reads the first one's row
            const long xr = ops.src_row(m);
            mean[u] = a.mean[m];
            rstd[u] = a.rstd[m];
            L.zero(xh[u]);
            L.zero(dy[u]);
            LN_FOR_CHUNKS(L, j, col) { ops.load(m, xr, col, xh[u][j], dy[u][j]); }
        }
        float c1[2] = {0.f, 0.f}, c2[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u)
            LN_FOR_CHUNKS(L, j, col) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xh[u][j][e] = (xh[u][j][e] - mean[u]) * rstd[u];
                    const float g = dy[u][j][e] * gam[j][e];
                    c1[u] += g;
                    c2[u] += g * xh[u][j][e];
                }
            }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) {      // four reductions interleaved
            c1[0] += __shfl_xor(c1[0], o, 64); c2[0] += __shfl_xor(c2[0], o, 64);
            c1[1] += __shfl_xor(c1[1], o, 64); c2[1] += __shfl_xor(c2[1], o, 64);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (mrow[u] >= a.M) continue;
            const int m = mrow[u];
            const float k1 = c1[u] * L.invD, k2 = c2[u] * L.invD;
            const long orow = ops.out_row(m);
            LN_FOR_CHUNKS(L, j, col) {
                f32x4 ds;
#pragma unroll
                for (int e = 0; e < 4; ++e) ds[e] = rstd[u] * (dy[u][j][e] * gam[j][e] - k1 - xh[u][j][e] * k2);
                if constexpr (Ops::adds_residual) ds = ops.residual(m, col) + ds;
                bf16x4 dsb;
                if constexpr (Ops::masks_out) dsb = round4(ops.mask_out(m, col, ds));     // (ds_f32 stays the residual's gradient)
                else dsb = round4(ds);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dg[j][e] += dy[u][j][e] * xh[u][j][e];
                    db[j][e] += dy[u][j][e];
                    dbi[j][e] += bf2f(dsb[e]);
                }
                store4(a.ds_f32, m, a.ds_bf16, orow, D, col, ds, dsb);
            }
        }
    }
    // column epilogue: sub-rows -> waves (LDS, wave order) -> workspace row or atomics
    if constexpr (L.RPW == 2) {                     // fold the two sub-rows of the wave before touching LDS
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dg[j][e] += __shfl_xor(dg[j][e], 32, 64);
                db[j][e] += __shfl_xor(db[j][e], 32, 64);
                dbi[j][e] += __shfl_xor(dbi[j][e], 32, 64);
            }
    }
    if (L.sr == 0)
        LN_FOR_CHUNKS(L, j, col) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                cacc[L.wave][0][col + e] = dg[j][e];
                cacc[L.wave][1][col + e] = db[j][e];
                cacc[L.wave][2][col + e] = dbi[j][e];
            }
        }
    __syncthreads();
    if (a.workspace) {   // plain coalesced stores of this workgroup's partials; a second kernel folds them
        float* ws = a.workspace + (long)blockIdx.x * 3 * D;
        for (int c = threadIdx.x; c < 3 * D; c += BWD_THREADS) {
            const int w = c / D, cc = c % D;
            ws[c] = cacc[0][w][cc] + cacc[1][w][cc] + cacc[2][w][cc] + cacc[3][w][cc];
        }
        return;
    }
    for (int c = threadIdx.x; c < D; c += BWD_THREADS) {
        if (a.dgamma) atomicAdd(a.dgamma + c, cacc[0][0][c] + cacc[1][0][c] + cacc[2][0][c] + cacc[3][0][c]);
        if (a.dbeta) atomicAdd(a.dbeta + c, cacc[0][1][c] + cacc[1][1][c] + cacc[2][1][c] + cacc[3][1][c]);
        if (a.dbias) atomicAdd(a.dbias + c, cacc[0][2][c] + cacc[1][2][c] + cacc[2][2][c] + cacc[3][2][c]);
    }
}

// post-norm: x-hat from x (+ r) through the input row remap, dy (+ dy2), ds_bf16 through the output row remap
struct PostNormBwd {
    static constexpr bool adds_residual = false, masks_out = false;
    const wj_ln_bwd_args a;
    __device__ __forceinline__ long src_row(int m) const {
        return remap_row(m, a.in_seg, a.in_valid, a.chan, a.chan > 1 ? a.M / (a.chan * a.in_valid) : 0);
    }
    __device__ __forceinline__ long out_row(int m) const {
        return remap_row(m, a.out_seg, a.out_valid, a.chan, a.chan > 1 ? a.M / (a.chan * a.out_valid) : 0);
    }
    __device__ __forceinline__ void load(int m, long xr, int col, f32x4& x, f32x4& dy) const {
        x = load4_sum(a.x, xr, a.x_is_bf16, a.r, m, a.D, col);
        dy = load4(a.dy, m, a.D, col, false);
        if (a.dy2) dy += load4(a.dy2, m, a.D, col, a.dy2_is_bf16);
    }
};
template <int V, int LPR>
__global__ __launch_bounds__(BWD_THREADS) void ln_bwd_kernel(wj_ln_bwd_args a) {
    ln_bwd_body<V, LPR>(PostNormBwd{a});
}

// post-norm under dropout of the addend r (wj_layernorm_bwd_drop): x-hat from x + r o m * scale; ds_bf16 = bf16(ds o m * scale) is the
// gradient of r.  The mask is regenerated in the load and in the store phase: held across the reductions it would cost registers.
struct PostNormDropBwd {
    static constexpr bool adds_residual = false, masks_out = true;
    const wj_ln_bwd_args a;
    const DropParams d;
    __device__ __forceinline__ long src_row(int m) const { return PostNormBwd{a}.src_row(m); }
    __device__ __forceinline__ long out_row(int m) const { return PostNormBwd{a}.out_row(m); }
    __device__ __forceinline__ void load(int m, long xr, int col, f32x4& x, f32x4& dy) const {
        x = load4_sum_drop(a.x, xr, a.x_is_bf16, a.r, m, a.D, col, d);
        dy = load4(a.dy, m, a.D, col, false);
        if (a.dy2) dy += load4(a.dy2, m, a.D, col, a.dy2_is_bf16);
    }
    __device__ __forceinline__ f32x4 mask_out(int m, int col, f32x4 ds) const { return drop4(ds, drop_bits4(d, m, a.D, col), d.scale); }
};
template <int V, int LPR>
__global__ __launch_bounds__(BWD_THREADS) void ln_bwd_drop_kernel(wj_ln_bwd_args a, DropParams d) {
    ln_bwd_body<V, LPR>(PostNormDropBwd{a, d});
}

// pre-norm: ds = (dres) + LN-backward(dy; s, gamma, mean, rstd).  dres is the gradient that bypasses the norm on the residual path (NULL
// behind a stack's final norm), dy the grad_input of the branch's first Linear (bf16 under autocast) or an f32 gradient.  One operand
// fewer than post-norm (the stream s was stored, there is no r to add back).  ds_bf16 = bf16(ds) is the dY of the PREVIOUS branch's last
// Linear and dbias its bias gradient.
struct PreNormBwd {
    static constexpr bool adds_residual = true, masks_out = false;
    const wj_ln_pre_bwd_args a;
    __device__ __forceinline__ long src_row(int m) const { return m; }
    __device__ __forceinline__ long out_row(int m) const { return m; }
    __device__ __forceinline__ void load(int m, long, int col, f32x4& s, f32x4& dy) const {
        s = load4(a.s, m, a.D, col, false);
        dy = load4(a.dy, m, a.D, col, a.dy_is_bf16);
    }
    // the residual-path gradient is read in the store phase, not with s and dy: held across the reductions it costs 8 V registers
    // (D = 768: 178 against 156, two waves per SIMD instead of three)
    __device__ __forceinline__ f32x4 residual(int m, int col) const {
        return a.dres ? load4(a.dres, m, a.D, col, false) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
};
template <int V, int LPR>
__global__ __launch_bounds__(BWD_THREADS) void ln_pre_bwd_kernel(wj_ln_pre_bwd_args a) {
    ln_bwd_body<V, LPR>(PreNormBwd{a});
}

// ---- column sums ------------------------------------------------------------------------------------------------------------------
// f32 tile: 128 columns [cb*128, +128) x rows [r0, r1) of x (float4 per thread, 8 row lanes).  Thread (cc, rl) adds rows r0 + rl,
// r0 + rl + 8, ... in ascending order, the eight row lanes are added in lane order, and add(o + c, s) takes the column's sum.  Columns
// [0, n_each) -> o0, [n_each, 2 n_each) -> o1, the rest -> o2 (LayerNorm's three gradients share one launch); NULL outputs are skipped.
template <class Add>
__device__ __forceinline__ void colsum_f32_tile(const float* x, long ldx, int r0, int r1, int N, int cb, float* o0, float* o1, float* o2,
                                                int n_each, Add add) {
    __shared__ float red[8][132];
    const int t = threadIdx.x, cc = t & 31, rl = t >> 5;
    const int col = cb * 128 + cc * 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < N)
        for (int r = r0 + rl; r < r1; r += 8) acc += *reinterpret_cast<const f32x4*>(x + (long)r * ldx + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rl][cc * 4 + e] = acc[e];
    __syncthreads();
    if (t < 128) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) s += red[r][t];
        const int c = cb * 128 + t;
        if (c < N) {
            const int which = c / n_each, cc2 = c - which * n_each;
            float* o = which == 0 ? o0 : (which == 1 ? o1 : o2);
            if (o) add(o + cc2, s);
        }
    }
}
// The two ways a tile's sum reaches out[c].  Atomic: row ranges of many workgroups meet in a float atomic.  Ordered (deterministic mode):
// ONE workgroup walks all rows of its columns and does out += s with a plain read-modify-write (stream-ordered behind whatever wrote
// `out` before) -- no float atomics, the result is a function of the inputs.  Meant for partial matrices of a few hundred rows (the
// LayerNorm / attention / scatter-fill partials, the second stage of the deterministic bf16 column sums).
struct AtomicAdd {
    __device__ __forceinline__ void operator()(float* p, float s) const { atomicAdd(p, s); }
};
struct OrderedAdd {
    __device__ __forceinline__ void operator()(float* p, float s) const { *p += s; }
};

// out[c] += sum over rows of an f32 matrix: workgroup = 128 columns x a row range
__global__ __launch_bounds__(256) void colsum_f32_kernel(const float* __restrict__ x, long ldx, int M, int N,
                                                         float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
                                                         int n_each, int rows_per_wg) {
    const int r0 = blockIdx.y * rows_per_wg;
    colsum_f32_tile(x, ldx, r0, min(M, r0 + rows_per_wg), N, blockIdx.x, o0, o1, o2, n_each, AtomicAdd{});
}
__global__ __launch_bounds__(256) void colsum_f32_det_kernel(const float* __restrict__ x, long ldx, int M, int N, float* o0, float* o1, float* o2,
                                                             int n_each) {
    colsum_f32_tile(x, ldx, 0, M, N, blockIdx.x, o0, o1, o2, n_each, OrderedAdd{});
}

// The same fold for up to WJ_COLSUM_GROUP_MAX matrices in ONE launch: the per-workgroup partials that the LayerNorm / attention backward
// kernels of a few layers left in their own scratch rows (wj_colsum_f32_group).  An item gets GROUP_CB x GROUP_RB workgroup slots
// (column blocks of 128 x row ranges; one row range when deterministic); slots beyond its width return at once.
constexpr int GROUP_CB = 18, GROUP_RB = 8;      // up to 2304 columns (3 x 768), 8 row ranges
__global__ __launch_bounds__(256) void colsum_f32_group_kernel(wj_colsum_group_args a) {
    const int item = blockIdx.x / (GROUP_CB * GROUP_RB), rem = blockIdx.x - item * (GROUP_CB * GROUP_RB);
    const int cb = rem % GROUP_CB, rb = rem / GROUP_CB;
    const int M = a.M[item], N = a.N[item];
    if (cb * 128 >= N) return;
    int rows = (M + GROUP_RB - 1) / GROUP_RB;
    rows = (rows + 7) / 8 * 8;
    const int r0 = rb * rows;
    if (r0 >= M) return;
    colsum_f32_tile(a.x[item], a.ldx[item], r0, min(M, r0 + rows), N, cb, a.o0[item], a.o1[item], a.o2[item], a.n_each[item], AtomicAdd{});
}
__global__ __launch_bounds__(256) void colsum_f32_group_det_kernel(wj_colsum_group_args a) {
    const int item = blockIdx.x / GROUP_CB, cb = blockIdx.x - item * GROUP_CB;
    if (cb * 128 >= a.N[item]) return;
    colsum_f32_tile(a.x[item], a.ldx[item], 0, a.M[item], a.N[item], cb, a.o0[item], a.o1[item], a.o2[item], a.n_each[item], OrderedAdd{});
}

// bf16 tile: workgroup = 64 columns x row range blockIdx.y; thread (cc = t&7 -> 8 columns, rl = t>>3 -> row lane of 32); put(c, s) takes
// the sum of column c
template <class Put>
__device__ __forceinline__ void colsum_bf16_tile(const wj_colsum_args& a, int rows_per_wg, Put put) {
    __shared__ float red[32][65];
    const int t = threadIdx.x, cc = t & 7, rl = t >> 3;
    const int col = blockIdx.x * 64 + cc * 8;
    const int r0 = blockIdx.y * rows_per_wg;
    const int r1 = min(a.M, r0 + rows_per_wg);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col < a.N) {
        for (int r = r0 + rl; r < r1; r += 32) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>((const bf16_t*)a.x + (long)r * a.ldx + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][cc * 8 + e] = acc[e];
    __syncthreads();
    if (t < 64) {
        float s = 0.f;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) s += red[r][t];
        const int c = blockIdx.x * 64 + t;
        if (c < a.N) put(c, s);
    }
}
__global__ __launch_bounds__(256) void colsum_kernel(wj_colsum_args a, int rows_per_wg) {
    colsum_bf16_tile(a, rows_per_wg, [&](int c, float s) { atomicAdd(a.out + c, s); });
}
// first stage of the deterministic bf16 column sums: row range y STORES its sums as row y of the workspace [gridDim.y][N]
__global__ __launch_bounds__(256) void colsum_partial_kernel(wj_colsum_args a, int rows_per_wg) {
    colsum_bf16_tile(a, rows_per_wg, [&](int c, float s) { a.workspace[(long)blockIdx.y * a.N + c] = s; });
}

void launch_colsum_f32(const float* x, long ldx, int M, int N, float* o0, float* o1, float* o2, int n_each, hipStream_t s) {
    const int gx = (N + 127) / 128;
    int gy = 1024 / gx;               // ~1000 workgroups: a thread sums only a handful of rows (latency-bound otherwise)
    if (gy < 1) gy = 1;
    if (gy > (M + 7) / 8) gy = (M + 7) / 8;
    int rows = (M + gy - 1) / gy;
    rows = (rows + 7) / 8 * 8;
    gy = (M + rows - 1) / rows;
    hipLaunchKernelGGL(colsum_f32_kernel, dim3(gx, gy), dim3(256), 0, s, x, ldx, M, N, o0, o1, o2, n_each, rows);
}
void launch_colsum_f32_det(const float* x, long ldx, int M, int N, float* o0, float* o1, float* o2, int n_each, hipStream_t s) {
    hipLaunchKernelGGL(colsum_f32_det_kernel, dim3((N + 127) / 128), dim3(256), 0, s, x, ldx, M, N, o0, o1, o2, n_each);
}
// row ranges of wj_colsum_bf16 (both forms): from M and N only
void colsum_bf16_plan(int M, int N, int& gx, int& gy, int& rows) {
    gx = (N + 63) / 64;
    gy = 2048 / gx;
    if (gy < 1) gy = 1;
    rows = (M + gy - 1) / gy;
    rows = (rows + 31) / 32 * 32;
    gy = (M + rows - 1) / rows;
}

// ---- host side: which <V, LPR> instance serves a width D, and the grids ---------------------------------------------------------------
template <int V_, int LPR_>
struct LnShape { static constexpr int V = V_, LPR = LPR_; };

bool ln_half(int D) { return (D % 128 == 0) && (D % 256 != 0) && D <= 384; }   // 128 / 384: 32 lanes per row

// f(LnShape<V, LPR>{}) for the instance of width D (D <= 256 * MAXV, checked by the entries)
template <class F>
void ln_dispatch(int D, F&& f) {
    if (ln_half(D)) {
        if (D == 128) f(LnShape<1, 32>{});
        else f(LnShape<3, 32>{});
        return;
    }
    switch ((D + 255) / 256) {
        case 1: f(LnShape<1, 64>{}); break;
        case 2: f(LnShape<2, 64>{}); break;
        case 3: f(LnShape<3, 64>{}); break;
        default: f(LnShape<4, 64>{}); break;
    }
}

// forward grid: four rows (eight at 32 lanes per row) per workgroup, or GS_SPLIT workgroups per row group
int ln_fwd_grid(int M, int D, bool grouped, int group_rows) {
    if (grouped) return ((M + group_rows - 1) / group_rows) * GS_SPLIT;
    const int rpw = ln_half(D) ? 2 : 1;
    const int grid = (M + 4 * rpw - 1) / (4 * rpw);
    return grid > 8192 ? 8192 : grid;
}

int ln_bwd_one_pass_rows() {   // WJ_LN_BWD_ONE_PASS_ROWS: launches of at most this many row slots give every wave ONE pass (0 = never)
    static const int v = wj_lab_env_int("WJ_LN_BWD_ONE_PASS_ROWS", 16384);
    return v;
}
// backward grid = the partial rows the backward leaves in its workspace ([rows][3][D]) for M token rows of width D
int ln_bwd_grid(int M, int D) {
    const int nw = BWD_THREADS / 64;
    const bool half = ln_half(D);
    const int rpw = half ? 2 : 1;
    // Large M: >= 8 rows per wave (4 passes of its two row slots) -- the per-workgroup epilogue (LDS fold, partials store) is paid once
    // per 32 rows and the chip is full anyway.  Small M (the ragged student's 10 k rows are 39 rows per CU): 314 such workgroups put
    // five waves on a CU, each running its four load -> reduce -> store round trips one after the other (51 us for 139 MB cold); with ONE
    // pass per wave there are 1256 workgroups, three resident per CU (150 VGPRs), and the launch takes 36 us (tools/ln_bench.py; 6 / 8
    // / 12-wave workgroups of one pass: 53 / 44 / 36 us -- what counts is how many waves of 150 VGPRs a CU holds, 12, and that they do
    // not all sit in the same phase).
    const int passes = (half ? (M + 1) / 2 : M) <= ln_bwd_one_pass_rows() ? 1 : 4;
    int grid = (M + 2 * passes * nw * rpw - 1) / (2 * passes * nw * rpw);
    return grid > LN_BWD_MAX_PARTIAL_ROWS ? LN_BWD_MAX_PARTIAL_ROWS : grid;
}

// launch of either backward kernel on ln_bwd_grid, then the fold of its workspace rows where gradient outputs are given
template <class Args, class Launch>
void ln_bwd_launch(const Args* a, hipStream_t s, Launch&& launch) {
    const int grid = ln_bwd_grid(a->M, a->D);
    ln_dispatch(a->D, [&](auto shape) { launch(shape, dim3(grid), dim3(BWD_THREADS)); });
    if (a->workspace && (a->dgamma || a->dbeta || a->dbias))
        launch_colsum_f32(a->workspace, 3L * a->D, grid, 3 * a->D, a->dgamma, a->dbeta, a->dbias, a->D, s);
}

}  // namespace

// partial-row bytes of the deterministic wj_colsum_bf16 -- wj_workspace_bytes("wj_colsum_bf16", args)
int64_t wj_colsum_bf16_ws_bytes(const wj_colsum_args* a) {
    if (!a || !a->deterministic || a->M <= 0 || a->N <= 0) return 0;
    int gx, gy, rows;
    colsum_bf16_plan(a->M, a->N, gx, gy, rows);
    return (int64_t)gy * a->N * 4;
}

static int ln_fwd_check(const wj_ln_fwd_args* a) {
    if (!a->x || !a->gamma || !a->beta) return WJ_ERR_ARG;
    if (a->M <= 0 || a->D <= 0 || (a->D & 3) || a->D > 256 * MAXV) return WJ_ERR_ARG;
    if (a->in_seg > 0 && a->in_valid <= 0) return WJ_ERR_ARG;
    if (a->in_chan > 1 && (a->in_seg <= 0 || a->M % (a->in_chan * a->in_valid))) return WJ_ERR_ARG;
    if (a->group_stats && a->group_rows <= 0) return WJ_ERR_ARG;
    if (a->y_fp8 && (!a->y_fp8_scales || (a->D % 128) || a->ld_fp8_scale < a->M)) return WJ_ERR_ARG;
    return WJ_OK;
}
static int ln_bwd_check(const wj_ln_bwd_args* a) {
    if (!a->dy || !a->x || !a->gamma || !a->mean || !a->rstd) return WJ_ERR_ARG;
    if (a->M <= 0 || a->D <= 0 || (a->D & 3) || a->D > 256 * MAXV) return WJ_ERR_ARG;
    if ((a->in_seg > 0 && a->in_valid <= 0) || (a->out_seg > 0 && a->out_valid <= 0)) return WJ_ERR_ARG;
    if (a->chan > 1 && ((a->in_seg > 0 && a->M % (a->chan * a->in_valid)) || (a->out_seg > 0 && a->M % (a->chan * a->out_valid)))) return WJ_ERR_ARG;
    return WJ_OK;
}

extern "C" int wj_layernorm_fwd(const wj_ln_fwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || ln_fwd_check(a) != WJ_OK) return WJ_ERR_ARG;
    const int grid = ln_fwd_grid(a->M, a->D, a->group_stats != nullptr, a->group_rows);
    hipStream_t s = (hipStream_t)stream;
    // the lean form on a capped grid (see ln_fwd_lean_kernel): same bits, a kernel that shares a CU with a persistent GEMM
    const bool lean = a->workgroups > 0 && !a->group_stats && !a->y_fp8 && a->in_seg <= 0;
    ln_dispatch(a->D, [&](auto shape) {
        using S = decltype(shape);
        if (lean) hipLaunchKernelGGL((ln_fwd_lean_kernel<S::V, S::LPR>), dim3(grid < a->workgroups ? grid : a->workgroups), dim3(256), 0, s, *a);
        else hipLaunchKernelGGL((ln_fwd_kernel<S::V, S::LPR>), dim3(grid), dim3(256), 0, s, *a);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

#ifdef WJ_DROPOUT_LIB
extern "C" WJ_EXPORT int wj_layernorm_fwd_drop(const wj_ln_fwd_drop_args* ad, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!ad) return WJ_ERR_ARG;
    const wj_ln_fwd_args* a = &ad->ln;
    DropParams d;
    if (ln_fwd_check(a) != WJ_OK || !a->r || (a->D & 7) || a->y_fp8 || !drop_params(ad->drop, d)) return WJ_ERR_ARG;
    const int grid = ln_fwd_grid(a->M, a->D, a->group_stats != nullptr, a->group_rows);
    hipStream_t s = (hipStream_t)stream;
    ln_dispatch(a->D, [&](auto shape) {
        using S = decltype(shape);
        hipLaunchKernelGGL((ln_fwd_drop_kernel<S::V, S::LPR>), dim3(grid), dim3(256), 0, s, *a, d);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
#endif

extern "C" int wj_ln_bwd_partial_rows(int M, int D) {
    if (M <= 0 || D <= 0) return -1;
    return ln_bwd_grid(M, D);
}
// workspace of either backward, sized for any M: the grid cap's partial rows
static int64_t ln_bwd_ws_bytes(int D) { return (int64_t)LN_BWD_MAX_PARTIAL_ROWS * 3 * D * 4; }
int64_t wj_ln_bwd_ws_bytes(const wj_ln_bwd_args* a) { return ln_bwd_ws_bytes(a->D); }
int64_t wj_ln_pre_bwd_ws_bytes(const wj_ln_pre_bwd_args* a) { return ln_bwd_ws_bytes(a->D); }
#ifdef WJ_DROPOUT_LIB
int64_t wj_ln_bwd_drop_ws_bytes(const wj_ln_bwd_drop_args* a) { return ln_bwd_ws_bytes(a->ln.D); }
#endif

extern "C" int wj_colsum_f32_group(const wj_colsum_group_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || a->n < 1 || a->n > WJ_COLSUM_GROUP_MAX) return WJ_ERR_ARG;
    for (int x = 0; x < a->n; ++x) {
        if (!a->x[x] || a->M[x] <= 0 || a->N[x] <= 0 || (a->N[x] & 3) || (a->ldx[x] & 3) || a->n_each[x] <= 0) return WJ_ERR_ARG;
        if (a->N[x] > GROUP_CB * 128 || a->N[x] > 3 * a->n_each[x]) return WJ_ERR_ARG;
    }
    if (a->deterministic) hipLaunchKernelGGL(colsum_f32_group_det_kernel, dim3(a->n * GROUP_CB), dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(colsum_f32_group_kernel, dim3(a->n * GROUP_CB * GROUP_RB), dim3(256), 0, (hipStream_t)stream, *a);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_layernorm_bwd(const wj_ln_bwd_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || ln_bwd_check(a) != WJ_OK) return WJ_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    ln_bwd_launch(a, s, [&](auto shape, dim3 g, dim3 b) {
        using S = decltype(shape);
        hipLaunchKernelGGL((ln_bwd_kernel<S::V, S::LPR>), g, b, 0, s, *a);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

#ifdef WJ_DROPOUT_LIB
extern "C" WJ_EXPORT int wj_layernorm_bwd_drop(const wj_ln_bwd_drop_args* ad, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!ad) return WJ_ERR_ARG;
    const wj_ln_bwd_args* a = &ad->ln;
    DropParams d;
    if (ln_bwd_check(a) != WJ_OK || !a->r || (a->D & 7) || !drop_params(ad->drop, d)) return WJ_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    ln_bwd_launch(a, s, [&](auto shape, dim3 g, dim3 b) {
        using S = decltype(shape);
        hipLaunchKernelGGL((ln_bwd_drop_kernel<S::V, S::LPR>), g, b, 0, s, *a, d);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
#endif

extern "C" int wj_layernorm_pre_fwd(const wj_ln_pre_fwd_args* a, void* stream) {
    if (!a || !a->x || !a->gamma || !a->beta) return WJ_ERR_ARG;
    if (a->M <= 0 || a->D <= 0 || (a->D & 3) || a->D > 256 * MAXV) return WJ_ERR_ARG;
    if (a->group_stats && a->group_rows <= 0) return WJ_ERR_ARG;
    WJ_CLEAR_STALE_ERROR();
    const int grid = ln_fwd_grid(a->M, a->D, a->group_stats != nullptr, a->group_rows);
    hipStream_t s = (hipStream_t)stream;
    ln_dispatch(a->D, [&](auto shape) {
        using S = decltype(shape);
        hipLaunchKernelGGL((ln_pre_fwd_kernel<S::V, S::LPR>), dim3(grid), dim3(256), 0, s, *a);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

// the backward runs on wj_layernorm_bwd's grid: the same partial rows
extern "C" int wj_ln_pre_bwd_partial_rows(int M, int D) { return wj_ln_bwd_partial_rows(M, D); }

extern "C" int wj_layernorm_pre_bwd(const wj_ln_pre_bwd_args* a, void* stream) {
    if (!a || !a->dy || !a->s || !a->gamma || !a->mean || !a->rstd) return WJ_ERR_ARG;
    if (a->M <= 0 || a->D <= 0 || (a->D & 3) || a->D > 256 * MAXV) return WJ_ERR_ARG;
    WJ_CLEAR_STALE_ERROR();
    hipStream_t s = (hipStream_t)stream;
    ln_bwd_launch(a, s, [&](auto shape, dim3 g, dim3 b) {
        using S = decltype(shape);
        hipLaunchKernelGGL((ln_pre_bwd_kernel<S::V, S::LPR>), g, b, 0, s, *a);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_colsum_f32(const wj_colsum_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || !a->x || !a->out || a->M <= 0 || a->N <= 0 || (a->N & 3) || (a->ldx & 3)) return WJ_ERR_ARG;
    if (a->deterministic) launch_colsum_f32_det((const float*)a->x, a->ldx, a->M, a->N, a->out, nullptr, nullptr, a->N, (hipStream_t)stream);
    else launch_colsum_f32((const float*)a->x, a->ldx, a->M, a->N, a->out, nullptr, nullptr, a->N, (hipStream_t)stream);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_colsum_bf16(const wj_colsum_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || !a->x || !a->out || a->M <= 0 || a->N <= 0 || (a->N & 7) || (a->ldx & 7)) return WJ_ERR_ARG;
    int gx, gy, rows;
    colsum_bf16_plan(a->M, a->N, gx, gy, rows);
    if (a->deterministic) {
        // two launches on the same stream: partial rows (plain stores), then one adder per column over them in row-range order
        if (!a->workspace || a->workspace_bytes < (int64_t)gy * a->N * 4 || ((uintptr_t)a->workspace & 15)) return WJ_ERR_ARG;
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, *a, rows);
        launch_colsum_f32_det(a->workspace, a->N, gy, a->N, a->out, nullptr, nullptr, a->N, (hipStream_t)stream);
        WJ_CHECK_LAUNCH();
        return WJ_OK;
    }
    hipLaunchKernelGGL(colsum_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, *a, rows);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
