// Conv front-end in mode="layer_norm" for gfx950: every conv layer is Conv1d(+bias) -> LayerNorm over channels -> erf-GELU.
// The activations are channels-last bf16 [rows][C], so the LayerNorm is a row LayerNorm.  One lane owns 8 consecutive channels (one
// 16-byte access), LPR = C / 8 lanes own a row (C = 512: a whole wave; C = 64: eight rows per wave), row sums are shuffles inside those
// lanes.  z = LN(pre) * gamma + beta exists in registers only: a layer costs 2 bytes in + 2 bytes out per element in the forward and
// 2 + 2 in + 2 out in the backward.
//   layers >= 1: `pre` comes from the conv GEMM (WJ_EPI_BF16 + bias); conv_ln_fwd / conv_ln_bwd stream over its rows.
//   layer 0:     C_in * k = 10 / 20 taps are no GEMM shape; conv0_ln_fwd / conv0_ln_bwd recompute the conv from the audio per row, the
//                lane's 8 x taps weights live in registers.
// Parameter gradients: every lane keeps its columns' sums in registers across its rows (a fixed row -> lane assignment), sub-rows are
// folded by shuffles, waves through LDS in wave order, and each workgroup STORES one partial row; the partial rows are added in row order
// by wj_colsum_f32_group (layers >= 1) or ordered_fold_kernel and conv0_ln_final_kernel (layer 0).  No float atomics anywhere in this file.
#include "conv_pieces.h"
#include "../../include/wavjepa_hip.h"

namespace {

constexpr int THREADS = 256, NW = THREADS / 64;

template <int LPR>
struct RowLanes {
    static constexpr int RPW = 64 / LPR;   // rows a wave works on at once
    static constexpr int C = LPR * 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & (LPR - 1), sr = lane / LPR;
    const int col = li * 8;
};

template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// adds the RPW sub-rows of a wave (kernel-uniform call, every lane active)
template <int LPR>
__device__ __forceinline__ float subrow_sum(float v) {
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p ? p[j] : 0.f;
}
__device__ __forceinline__ void unpack8(const bf16x8 b, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(b[j]);
}
__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = f2bf(0.f);
    return z;
}

// mean and rstd of the lane group's row from its 8 values: the mean first, then the squared deviations (biased variance)
template <int LPR>
__device__ __forceinline__ void row_stats(const float (&x)[8], float eps, float& mean, float& rstd) {
    constexpr float invC = 1.0f / (float)(LPR * 8);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += x[j];
    mean = row_sum<LPR>(s) * invC;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float d = x[j] - mean;
        sq = fmaf(d, d, sq);
    }
    rstd = rsqrtf(row_sum<LPR>(sq) * invC + eps);
}

// post = bf16(gelu(xh * gamma + beta)) of one row
__device__ __forceinline__ bf16x8 ln_gelu8(const float (&x)[8], float mean, float rstd, const float (&gam)[8], const float (&bet)[8]) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(gelu_f(fmaf((x[j] - mean) * rstd, gam[j], bet[j])));
    return o;
}

// Backward of GELU and LayerNorm for one row: x = the row's pre-activations, d = its output gradient.  Returns dpre (fp32) in `dx` and adds
// the row's terms to the lane's dgamma / dbeta sums.
template <int LPR>
__device__ __forceinline__ void ln_gelu_bwd8(const float (&x)[8], const float (&d)[8], float mean, float rstd, const float (&gam)[8],
                                             const float (&bet)[8], float (&dx)[8], float (&dg)[8], float (&db)[8]) {
    constexpr float invC = 1.0f / (float)(LPR * 8);
    float xh[8], gg[8], c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        xh[j] = (x[j] - mean) * rstd;
        const float g = d[j] * gelu_grad_f(fmaf(xh[j], gam[j], bet[j]));
        dg[j] = fmaf(g, xh[j], dg[j]);
        db[j] += g;
        gg[j] = g * gam[j];
        c1 += gg[j];
        c2 = fmaf(gg[j], xh[j], c2);
    }
    c1 = row_sum<LPR>(c1) * invC;
    c2 = row_sum<LPR>(c2) * invC;
#pragma unroll
    for (int j = 0; j < 8; ++j) dx[j] = rstd * (gg[j] - c1 - xh[j] * c2);
}

// ---- layers >= 1 -------------------------------------------------------------------------------------------------------------------
template <int LPR>
__global__ __launch_bounds__(THREADS) void conv_ln_fwd_kernel(wj_conv_ln_fwd_args a) {
    const RowLanes<LPR> L;
    constexpr int C = RowLanes<LPR>::C, RPW = RowLanes<LPR>::RPW;
    float gam[8], bet[8];
    load8(a.gamma + L.col, gam);
    load8(a.beta + L.col, bet);
    const int stride = gridDim.x * NW * RPW;
    for (int m = (blockIdx.x * NW + L.wave) * RPW + L.sr; m < a.M; m += stride) {
        bf16x8* dst = reinterpret_cast<bf16x8*>((bf16_t*)a.post + (long)m * C + L.col);
        if (a.seg_rows > 0 && (m % a.seg_rows) >= a.seg_valid) {      // clip padding: written as 0, `pre` is not read
            *dst = zero8();
            if (L.li == 0) {
                if (a.mean) a.mean[m] = 0.f;
                if (a.rstd) a.rstd[m] = 0.f;
            }
            continue;
        }
        float x[8], mean, rstd;
        unpack8(*reinterpret_cast<const bf16x8*>((const bf16_t*)a.pre + (long)m * C + L.col), x);
        row_stats<LPR>(x, a.eps, mean, rstd);
        *dst = ln_gelu8(x, mean, rstd, gam, bet);
        if (L.li == 0) {
            if (a.mean) a.mean[m] = mean;
            if (a.rstd) a.rstd[m] = rstd;
        }
    }
}

// total = rows processed: M (dense) or n_rows (listed).  Every workgroup stores its partial row [3][C], also one without rows.
template <int LPR>
__global__ __launch_bounds__(THREADS) void conv_ln_bwd_kernel(wj_conv_ln_bwd_args a, int total) {
    const RowLanes<LPR> L;
    constexpr int C = RowLanes<LPR>::C, RPW = RowLanes<LPR>::RPW;
    __shared__ float cacc[NW][3][C];
    float gam[8], bet[8], dg[8], db[8], dbi[8];
    load8(a.gamma + L.col, gam);
    load8(a.beta + L.col, bet);
    load8(nullptr, dg);
    load8(nullptr, db);
    load8(nullptr, dbi);
    const int stride = gridDim.x * NW * RPW;
    for (int i = (blockIdx.x * NW + L.wave) * RPW + L.sr; i < total; i += stride) {
        const int m = a.rows ? a.rows[i] : i;
        if ((unsigned)m >= (unsigned)a.M) continue;
        const long at = (long)m * C + L.col;
        bf16x8* dpost = reinterpret_cast<bf16x8*>((bf16_t*)a.dpost + at);
        bf16x8* dpre = reinterpret_cast<bf16x8*>((bf16_t*)a.dpre + at);
        if (a.seg_rows > 0 && (m % a.seg_rows) >= a.seg_valid) {      // clip padding: no gradient, nothing read
            *dpre = zero8();
            if (a.clear_dpost) *dpost = zero8();
            continue;
        }
        float x[8], d[8], dx[8];
        unpack8(*reinterpret_cast<const bf16x8*>((const bf16_t*)a.pre + at), x);
        unpack8(*dpost, d);
        ln_gelu_bwd8<LPR>(x, d, a.mean[m], a.rstd[m], gam, bet, dx, dg, db);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = f2bf(dx[j]);
            dbi[j] += bf2f(o[j]);
        }
        *dpre = o;
        if (a.clear_dpost) *dpost = zero8();
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        dg[j] = subrow_sum<LPR>(dg[j]);
        db[j] = subrow_sum<LPR>(db[j]);
        dbi[j] = subrow_sum<LPR>(dbi[j]);
    }
    if (L.sr == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            cacc[L.wave][0][L.col + j] = dg[j];
            cacc[L.wave][1][L.col + j] = db[j];
            cacc[L.wave][2][L.col + j] = dbi[j];
        }
    }
    __syncthreads();
    float* ws = a.workspace + (long)blockIdx.x * 3 * C;
    for (int c = threadIdx.x; c < 3 * C; c += THREADS) {
        const int w = c / C, cc = c - w * C;
        ws[c] = cacc[0][w][cc] + cacc[1][w][cc] + cacc[2][w][cc] + cacc[3][w][cc];
    }
}

int bwd_grid(int rows, int C) {
    const int per_wg = NW * (512 / C) * 4;       // four passes of a workgroup's row slots
    int grid = (rows + per_wg - 1) / per_wg;
    grid = grid < 1 ? 1 : grid;
    return grid > LN_BWD_MAX_PARTIAL_ROWS ? LN_BWD_MAX_PARTIAL_ROWS : grid;   // the partial rows fit the scratch wj_layernorm_bwd's callers hold
}

bool width_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// f(lanes-per-row constant) for the supported widths
template <class F>
void width_dispatch(int C, F&& f) {
    switch (C) {
        case 64: f(std::integral_constant<int, 8>{}); break;
        case 128: f(std::integral_constant<int, 16>{}); break;
        case 256: f(std::integral_constant<int, 32>{}); break;
        default: f(std::integral_constant<int, 64>{}); break;
    }
}

// ---- layer 0 -----------------------------------------------------------------------------------------------------------------------
template <int LPR, int TAPS>
__global__ __launch_bounds__(THREADS) void conv0_ln_fwd_kernel(wj_conv0_ln_fwd_args a, long clip_stride) {
    const RowLanes<LPR> L;
    constexpr int C = RowLanes<LPR>::C, RPW = RowLanes<LPR>::RPW;
    float w[8][TAPS], bi[8], gam[8], bet[8];
    load_weights(w, (const bf16_t*)a.w, L.col);
    load8(a.bias ? a.bias + L.col : nullptr, bi);
    load8(a.gamma + L.col, gam);
    load8(a.beta + L.col, bet);
    int off[TAPS];
    tap_offsets(off, a.k, a.L);
    const int total = a.N * a.P, stride = gridDim.x * NW * RPW;
    for (int r = (blockIdx.x * NW + L.wave) * RPW + L.sr; r < total; r += stride) {
        const int n = r / a.P, t = r - n * a.P;
        bf16x8* dst = reinterpret_cast<bf16x8*>((bf16_t*)a.act + (long)r * C + L.col);
        if (t >= a.L_out) {
            *dst = zero8();
            if (L.li == 0) {
                a.mean[r] = 0.f;
                a.rstd[r] = 0.f;
            }
            continue;
        }
        const bf16_t* ap = (const bf16_t*)a.audio + (long)n * clip_stride + (long)t * a.stride;
        float x[TAPS], y[8], mean, rstd;
        load_patch(x, ap, off);
        conv_row(y, x, [&](int j, int q) { return w[j][q]; }, bi);
        row_stats<LPR>(y, a.eps, mean, rstd);
        *dst = ln_gelu8(y, mean, rstd, gam, bet);
        if (L.li == 0) {
            a.mean[r] = mean;
            a.rstd[r] = rstd;
        }
    }
}

// Workgroup (chunk, clip): up to BR0 rows of one clip -- listed rows [row_off[n] + chunk * BR0, ...) or time steps chunk * BR0 ... -- and ONE
// partial record  [C][TAPS] dw | [C] dbias | [C] dgamma | [C] dbeta  stored at part[n][chunk] (zeros when the clip has no row there).
constexpr int BR0 = 512;
__host__ __device__ constexpr int64_t record_floats(int C, int taps) { return (int64_t)C * (taps + 3); }

template <int LPR, int TAPS>
__global__ __launch_bounds__(THREADS) void conv0_ln_bwd_kernel(wj_conv0_ln_bwd_args a, long clip_stride, float* __restrict__ part) {
    const RowLanes<LPR> L;
    constexpr int C = RowLanes<LPR>::C, RPW = RowLanes<LPR>::RPW, REC = record_floats(C, TAPS);
    __shared__ float racc[REC];
    bf16x2 w2[8][TAPS / 2];                      // the lane's weights, two taps per register
    float bi[8], gam[8], bet[8], dw[8][TAPS], dbs[8], dg[8], db[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < TAPS; q += 2)
            w2[j][q / 2] = *reinterpret_cast<const bf16x2*>((const bf16_t*)a.w + (long)(L.col + j) * TAPS + q);
    load8(a.bias ? a.bias + L.col : nullptr, bi);
    load8(a.gamma + L.col, gam);
    load8(a.beta + L.col, bet);
    load8(nullptr, dbs);
    load8(nullptr, dg);
    load8(nullptr, db);
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < TAPS; ++q) dw[j][q] = 0.f;
    int off[TAPS];
    tap_offsets(off, a.k, a.L);
    const int n = blockIdx.y;
    const int first = a.rows ? a.row_off[n] : 0;
    const int cnt = a.rows ? a.row_off[n + 1] - first : a.L_out;
    const int j0 = blockIdx.x * BR0;
    const int jn = min(BR0, cnt - j0);           // <= 0: no row of this clip in this chunk
    for (int jr = L.wave * RPW + L.sr; jr < jn; jr += NW * RPW) {
        const int t = a.rows ? a.rows[first + j0 + jr] - n * a.P : j0 + jr;
        if ((unsigned)t >= (unsigned)a.L_out) continue;
        const long r = (long)n * a.P + t;
        const bf16_t* ap = (const bf16_t*)a.audio + (long)n * clip_stride + (long)t * a.stride;
        float x[TAPS], y[8], d[8], dx[8];
        load_patch(x, ap, off);
        unpack8(*reinterpret_cast<const bf16x8*>((const bf16_t*)a.dact + r * C + L.col), d);
        conv_row(y, x, [&](int j, int q) { return bf2f(w2[j][q / 2][q & 1]); }, bi);
        ln_gelu_bwd8<LPR>(y, d, a.mean[r], a.rstd[r], gam, bet, dx, dg, db);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float dy = bf2f(f2bf(dx[j]));  // the conv output's gradient is a bf16 tensor, as d(pre) of the layers above
            dbs[j] += dy;
#pragma unroll
            for (int q = 0; q < TAPS; ++q) dw[j][q] = fmaf(dy, x[q], dw[j][q]);
        }
    }
    // sub-rows by shuffles, then the four waves into LDS one after the other (wave order)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        dbs[j] = subrow_sum<LPR>(dbs[j]);
        dg[j] = subrow_sum<LPR>(dg[j]);
        db[j] = subrow_sum<LPR>(db[j]);
#pragma unroll
        for (int q = 0; q < TAPS; ++q) dw[j][q] = subrow_sum<LPR>(dw[j][q]);
    }
    for (int wv = 0; wv < NW; ++wv) {
        if (L.wave == wv && L.sr == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = L.col + j;
#pragma unroll
                for (int q = 0; q < TAPS; ++q) racc[c * TAPS + q] = (wv ? racc[c * TAPS + q] : 0.f) + dw[j][q];
                racc[C * TAPS + c] = (wv ? racc[C * TAPS + c] : 0.f) + dbs[j];
                racc[C * (TAPS + 1) + c] = (wv ? racc[C * (TAPS + 1) + c] : 0.f) + dg[j];
                racc[C * (TAPS + 2) + c] = (wv ? racc[C * (TAPS + 2) + c] : 0.f) + db[j];
            }
        }
        __syncthreads();
    }
    float* o = part + ((long)n * gridDim.x + blockIdx.x) * REC;
    for (int i = threadIdx.x; i < REC; i += THREADS) o[i] = racc[i];
}

// gradient += sum over clips, in clip order, of folded[n][i]; one thread owns an element: a plain accumulate into the gradient buffers
__global__ __launch_bounds__(256) void conv0_ln_final_kernel(const float* __restrict__ folded, int N, int C, int taps, float* __restrict__ dw,
                                                             float* __restrict__ dbias, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int rec = C * (taps + 3);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rec) return;
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += folded[(long)n * rec + i];
    const int nw = C * taps;
    if (i < nw) dw[i] += s;
    else if (i < nw + C) { if (dbias) dbias[i - nw] += s; }
    else if (i < nw + 2 * C) dgamma[i - nw - C] += s;
    else dbeta[i - nw - 2 * C] += s;
}

int conv0_chunks(int L_out, int max_rows) { return ((max_rows > 0 ? max_rows : L_out) + BR0 - 1) / BR0; }

template <int LPR, int TAPS>
void launch_conv0_bwd(const wj_conv0_ln_bwd_args* a, long clip_stride, hipStream_t s) {
    constexpr int C = LPR * 8, REC = record_floats(C, TAPS);
    const int chunks = conv0_chunks(a->L_out, a->rows ? a->max_rows : 0);
    float* folded = a->workspace;                         // [N][REC]
    float* part = a->workspace + (long)a->N * REC;        // [N][chunks][REC]
    hipLaunchKernelGGL((conv0_ln_bwd_kernel<LPR, TAPS>), dim3(chunks, a->N), dim3(THREADS), 0, s, *a, clip_stride, part);
    fold_records(s, (REC + 255) / 256, a->N, (const float*)part, chunks, REC, folded, REC);
    hipLaunchKernelGGL(conv0_ln_final_kernel, dim3((REC + 255) / 256), dim3(256), 0, s, (const float*)folded, a->N, C, TAPS, a->dw, a->dbias,
                       a->dgamma, a->dbeta);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// geometry of the two layer-0 entries (`rows16` = the [N * P][C] tensor the entry streams); args_ok = the entry's own argument rules
template <class A>
int layer0_check(const A* a, const void* rows16, bool args_ok = true) {
    if (a->N <= 0 || a->C <= 0 || a->C_in <= 0 || a->k <= 0 || a->stride <= 0 || a->L_out <= 0 || a->P < a->L_out || !aligned16(rows16)) return WJ_ERR_ARG;
    if ((long)(a->L_out - 1) * a->stride + a->k > a->L || (long)a->N * a->P >= (1L << 31)) return WJ_ERR_ARG;
    if (a->audio_clip_stride != 0 && a->audio_clip_stride < (int64_t)a->C_in * a->L) return WJ_ERR_ARG;
    if (!args_ok) return WJ_ERR_ARG;
    return width_ok(a->C) && taps_ok(a->C_in * a->k) ? WJ_OK : WJ_ERR_UNSUPPORTED;
}

}  // namespace

// scratch of wj_conv0_ln_gelu_bwd -- wj_workspace_bytes("wj_conv0_ln_gelu_bwd", args): folded [N][rec] + partial records [N][chunks][rec]
int64_t wj_conv0_ln_bwd_ws_bytes(const wj_conv0_ln_bwd_args* a) {
    if (!a || a->N <= 0 || a->C <= 0 || a->C_in <= 0 || a->k <= 0 || a->L_out <= 0 || a->max_rows < 0) return -1;
    return (int64_t)a->N * (1 + conv0_chunks(a->L_out, a->max_rows)) * record_floats(a->C, a->C_in * a->k) * 4;
}

extern "C" int wj_conv_ln_gelu_fwd(const wj_conv_ln_fwd_args* a, void* stream) {
    if (!a || !a->pre || !a->gamma || !a->beta || !a->post) return WJ_ERR_ARG;
    if (a->M <= 0 || a->C <= 0 || !aligned16(a->pre) || !aligned16(a->post)) return WJ_ERR_ARG;
    if (a->seg_rows < 0 || (a->seg_rows > 0 && (a->seg_valid <= 0 || a->seg_valid > a->seg_rows))) return WJ_ERR_ARG;
    if (!width_ok(a->C)) return WJ_ERR_UNSUPPORTED;
    WJ_CLEAR_STALE_ERROR();
    width_dispatch(a->C, [&](auto lpr) {
        hipLaunchKernelGGL((conv_ln_fwd_kernel<decltype(lpr)::value>), dim3(row_grid(a->M, NW * (512 / a->C))), dim3(THREADS), 0, (hipStream_t)stream, *a);
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_conv_ln_bwd_partial_rows(int rows, int C) {
    if (rows < 0 || !width_ok(C)) return -1;
    return bwd_grid(rows, C);
}
// workspace of wj_conv_ln_gelu_bwd: its partial rows [rows][3][C]
int64_t wj_conv_ln_bwd_ws_bytes(const wj_conv_ln_bwd_args* a) {
    const int rows = wj_conv_ln_bwd_partial_rows(a->rows ? a->n_rows : a->M, a->C);
    return rows < 0 ? -1 : (int64_t)rows * 3 * a->C * 4;
}

extern "C" int wj_conv_ln_gelu_bwd(const wj_conv_ln_bwd_args* a, void* stream) {
    if (!a || !a->dpost || !a->pre || !a->mean || !a->rstd || !a->gamma || !a->beta || !a->dpre || !a->workspace) return WJ_ERR_ARG;
    if (a->M <= 0 || a->C <= 0 || !aligned16(a->pre) || !aligned16(a->dpost) || !aligned16(a->dpre)) return WJ_ERR_ARG;
    if (a->seg_rows < 0 || (a->seg_rows > 0 && (a->seg_valid <= 0 || a->seg_valid > a->seg_rows))) return WJ_ERR_ARG;
    if (a->rows && a->n_rows < 0) return WJ_ERR_ARG;
    if (!width_ok(a->C)) return WJ_ERR_UNSUPPORTED;
    WJ_CLEAR_STALE_ERROR();
    const int total = a->rows ? a->n_rows : a->M;
    const int grid = bwd_grid(total, a->C);
    width_dispatch(a->C, [&](auto lpr) {
        hipLaunchKernelGGL((conv_ln_bwd_kernel<decltype(lpr)::value>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, *a, total);
    });
    WJ_CHECK_LAUNCH();
    if (a->dgamma || a->dbeta || a->dbias) {
        wj_colsum_group_args f = {};
        f.n = 1;
        f.deterministic = a->deterministic;
        f.x[0] = a->workspace; f.ldx[0] = 3L * a->C; f.M[0] = grid; f.N[0] = 3 * a->C; f.n_each[0] = a->C;
        f.o0[0] = a->dgamma; f.o1[0] = a->dbeta; f.o2[0] = a->dbias;
        return wj_colsum_f32_group(&f, stream);
    }
    return WJ_OK;
}

extern "C" int wj_conv0_ln_gelu_fwd(const wj_conv0_ln_fwd_args* a, void* stream) {
    if (!a || !a->audio || !a->w || !a->gamma || !a->beta || !a->act || !a->mean || !a->rstd) return WJ_ERR_ARG;
    if (const int bad = layer0_check(a, a->act)) return bad;
    WJ_CLEAR_STALE_ERROR();
    const long clip_stride = packed_clip_stride(a->audio_clip_stride, a->C_in, a->L);
    const unsigned grid = row_grid((long)a->N * a->P, NW * (512 / a->C));
    width_dispatch(a->C, [&](auto lpr) {
        taps_dispatch(a->C_in * a->k, [&](auto taps) {
            hipLaunchKernelGGL((conv0_ln_fwd_kernel<decltype(lpr)::value, decltype(taps)::value>), dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, *a,
                               clip_stride);
        });
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

extern "C" int wj_conv0_ln_gelu_bwd(const wj_conv0_ln_bwd_args* a, void* stream) {
    if (!a || !a->audio || !a->w || !a->gamma || !a->beta || !a->mean || !a->rstd || !a->dact || !a->dw || !a->dgamma || !a->dbeta ||
        !a->workspace)
        return WJ_ERR_ARG;
    const bool lists_ok = !a->rows || (a->row_off && a->max_rows >= 0);
    if (const int bad = layer0_check(a, a->dact, lists_ok && (bool)a->bias == (bool)a->dbias)) return bad;
    if (a->rows && a->max_rows == 0) return WJ_OK;        // no listed row in any clip: nothing to add
    WJ_CLEAR_STALE_ERROR();
    const long clip_stride = packed_clip_stride(a->audio_clip_stride, a->C_in, a->L);
    width_dispatch(a->C, [&](auto lpr) {
        taps_dispatch(a->C_in * a->k, [&](auto taps) { launch_conv0_bwd<decltype(lpr)::value, decltype(taps)::value>(a, clip_stride, (hipStream_t)stream); });
    });
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}
