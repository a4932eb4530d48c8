// HBM-bound plumbing kernels of the WavJEPA step for gfx950: token gather/scatter, positions, conv weight layouts,
// GELU backward, teacher targets (joint instance norm), masked MSE, EMA, AdamW (+ global-norm clip), casts and the
// crop/normalise batch preparation.  All are vectorised (8-16 B per lane) streaming kernels or small reductions.
#include "stream_pieces.h"
#ifdef WJ_LAB
#include "../../include/wavjepa_hip_lab.h"
#endif

namespace {

// ------------------------------------------------------------------------------------------- GELU backward (bf16)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const bf16_t* __restrict__ dpost, const bf16_t* __restrict__ pre,
                                                       bf16_t* __restrict__ dpre, long n8) {
    for_each_flat(n8, [&](long i) {
        *reinterpret_cast<bf16x8*>(dpre + i * 8) =
            gelu_bwd8(*reinterpret_cast<const bf16x8*>(dpost + i * 8), *reinterpret_cast<const bf16x8*>(pre + i * 8));
    });
}

// listed rows only (sparse conv backward); the consumed dpost rows are zeroed on the way (clear_dpost) so that the buffer
// is all-zero again for the next step
__global__ __launch_bounds__(256) void gelu_bwd_rows_kernel(bf16_t* __restrict__ dpost, const bf16_t* __restrict__ pre,
                                                            bf16_t* __restrict__ dpre, const int32_t* __restrict__ rows,
                                                            int n_rows, int row8, int clear_dpost) {
    for_each_row_col(n_rows, row8, [&](int r, int c) {
        const long off = ((long)rows[r] * row8 + c) * 8;
        *reinterpret_cast<bf16x8*>(dpre + off) =
            gelu_bwd8(*reinterpret_cast<const bf16x8*>(dpost + off), *reinterpret_cast<const bf16x8*>(pre + off));
        if (clear_dpost) *reinterpret_cast<bf16x8*>(dpost + off) = bf16x8{};
    });
}

__global__ __launch_bounds__(256) void zero_rows_kernel(char* __restrict__ buf, const int32_t* __restrict__ rows, int n_rows,
                                                        int row16) {
    for_each_row_col(n_rows, row16, [&](int r, int c) {
        *reinterpret_cast<uint4*>(buf + ((long)rows[r] * row16 + c) * 16) = make_uint4(0, 0, 0, 0);
    });
}

// ------------------------------------------------------------------------------------------- conv weight layouts
__global__ __launch_bounds__(256) void conv_w_kernel(wj_conv_w_args a) {
    const int Co = a.C_out, Ci = a.C_in, k = a.k;
    if (a.mode == 0) {  // wp[o][kk*Ci + c] = w[o][c][kk]
        for_each_flat((long)Co * Ci * k, [&](long i) {
            const int c = (int)(i % Ci);
            const int kk = (int)((i / Ci) % k);
            const int o = (int)(i / ((long)Ci * k));
            ((bf16_t*)a.dst)[i] = f2bf(((const float*)a.src)[((long)o * Ci + c) * k + kk]);
        });
    } else if (a.mode == 1) {  // wd[v*Co + o][c] = w[o][c][rho + stride*(U-1-v)]
        for_each_flat((long)a.U * Co * Ci, [&](long i) {
            const int c = (int)(i % Ci);
            const int o = (int)((i / Ci) % Co);
            const int v = (int)(i / ((long)Ci * Co));
            const int kk = a.rho + a.stride * (a.U - 1 - v);
            ((bf16_t*)a.dst)[i] = f2bf(((const float*)a.src)[((long)o * Ci + c) * k + kk]);
        });
    } else {  // dw[o][c][kk] += dwp[o][kk*Ci + c]
        for_each_flat((long)Co * Ci * k, [&](long i) {
            const int kk = (int)(i % k);
            const int c = (int)((i / k) % Ci);
            const int o = (int)(i / ((long)Ci * k));
            ((float*)a.dst)[i] += ((const float*)a.src)[(long)o * Ci * k + (long)kk * Ci + c];
        });
    }
}

// ------------------------------------------------------------------------------------------- + positions
__global__ __launch_bounds__(256) void add_pos_kernel(wj_add_pos_args a) {
    for_each_row_col(a.M, a.D / 4, [&](int m, int c4) {
        const int c = c4 * 4;
        const f32x4 y = to_f32x4(*reinterpret_cast<const bf16x4*>((const bf16_t*)a.x + (long)m * a.D + c)) +
                        *reinterpret_cast<const f32x4*>(a.pos + (long)(m % a.T) * a.D + c);
        if (a.y_f32) *reinterpret_cast<f32x4*>(a.y_f32 + (long)m * a.D + c) = y;
        if (a.y_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.y_bf16 + (long)m * a.D + c) = to_bf16x4(y);
    });
}

// ------------------------------------------------------------------------------------------- mask gather (bit-exact copy)
__global__ __launch_bounds__(256) void gather_rows_kernel(const char* __restrict__ x, const int32_t* __restrict__ idx,
                                                          char* __restrict__ out, int n_rows, int row_bytes) {
    const int chunks = row_bytes / 16;
    for (int j = blockIdx.x; j < n_rows; j += gridDim.x) {
        const char* s = x + (long)idx[j] * row_bytes;
        char* d = out + (long)j * row_bytes;
        for (int c = threadIdx.x; c < chunks; c += 256)
            *reinterpret_cast<uint4*>(d + c * 16) = *reinterpret_cast<const uint4*>(s + c * 16);
    }
}

// ------------------------------------------------------------------------------------------- predictor input
__global__ __launch_bounds__(256) void scatter_fill_kernel(wj_scatter_fill_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D, M = a.B * a.T;
    for (int m = blockIdx.x * 4 + wave; m < M; m += gridDim.x * 4) {
        const int b = m / a.T, t = m - b * a.T;
        const int src = a.inv[m];
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 y;
            bf16x4 yb;
            fill_token(a, src, t, c, y, yb);
            for (int g = 0; g < a.G; ++g) {
                const long orow = ((long)b * a.G + g) * a.T + t;
                if (a.out_f32) *reinterpret_cast<f32x4*>(a.out_f32 + orow * D + c) = y;
                if (a.out_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.out_bf16 + orow * D + c) = yb;
            }
        }
    }
}

// ragged form: one packed output row per listed dense index (b*G+g)*T + t
__global__ __launch_bounds__(256) void scatter_fill_rows_kernel(wj_scatter_fill_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D;
    for (int r = blockIdx.x * 4 + wave; r < a.n_rows; r += gridDim.x * 4) {
        const int dense = a.rows[r];
        const int bg = dense / a.T, t = dense - bg * a.T, b = bg / a.G;
        const int src = a.inv[b * a.T + t];
        for (int c = lane * 4; c < D; c += 256) {
            f32x4 y;
            bf16x4 yb;
            fill_token(a, src, t, c, y, yb);
            if (a.out_f32) *reinterpret_cast<f32x4*>(a.out_f32 + (long)r * D + c) = y;
            if (a.out_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.out_bf16 + (long)r * D + c) = yb;
        }
    }
}

// Backward.  Round 4's form (64 rows per workgroup, a wave walking 16 rows one after the other: index load -> row-map load -> data
// load, three dependent round trips per row, then 384 global float atomics per workgroup into the same 384 addresses) ran at
// 1.4 TB/s.  Now a wave owns SFB_WROWS rows whose indices (inv, and the G row-map entries of each) are fetched up front by one load per
// lane and handed round with readlane; the G x SFB_WROWS data loads then have no address dependence on each other.  The mask-token
// gradient of a workgroup goes to a row of `partials` (no atomics; folded by wj_colsum_f32_group) when the caller gives one.
constexpr int SFB_WROWS = 4;                 // rows per wave
constexpr int SFB_ROWS = 4 * SFB_WROWS;      // rows per workgroup
// JMAX: 256-float column blocks a lane may own (2: D <= 512 -- half the registers, so that two waves per SIMD fit beside a weight-gradient
// workgroup of the other stream, which is what this kernel runs against on the main stream's critical path; 4: D <= 1024)
template <int JMAX>
__global__ __launch_bounds__(256) void scatter_fill_bwd_kernel(wj_scatter_fill_bwd_args a) {
    // [4 waves][D] floats, sized at launch: a fixed [4][1024] (16 KB) left room for two of these workgroups beside a weight-gradient
    // workgroup of the other stream (128 KB of a CU's 160) and the kernel, on the main stream's critical path, ran 405 us instead of 90
    extern __shared__ float macc_dyn[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = a.D, M = a.B * a.T, G = a.G;
    const int m0 = blockIdx.x * SFB_ROWS + wave * SFB_WROWS;
    // lane l < SFB_WROWS * (G + 1): row r = l / (G + 1), slot u = l % (G + 1): u == G -> inv[m], else the (packed) input row of group u
    int idx = -1;
    {
        const int r = lane / (G + 1), u = lane - r * (G + 1), m = m0 + r;
        if (r < SFB_WROWS && m < M) {
            if (u == G) {
                idx = a.inv[m];
            } else {
                const int b = m / a.T, t = m - b * a.T;
                const int row = (b * G + u) * a.T + t;
                idx = a.rowmap ? a.rowmap[row] : row;          // ragged: packed row of this token, -1 = not visible
            }
        }
    }
    f32x4 mt[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) mt[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < SFB_WROWS; ++r) {
        if (m0 + r >= M) break;
        const int dst = __builtin_amdgcn_readlane(idx, r * (G + 1) + G);
        f32x4 s[JMAX];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // four groups at a time, branch-free: every load of the batch is issued before the first add (with a `continue` on invisible
        // rows the loads of successive groups were separated by control flow -- one memory round trip per group and row)
        for (int g0 = 0; g0 < G; g0 += 4) {
            f32x4 v[4][JMAX];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int g = g0 + u;
                const int row = g < G ? __builtin_amdgcn_readlane(idx, r * (G + 1) + (g < G ? g : 0)) : -1;
                ok[u] = row >= 0;
                const float* src = a.d_in + (long)(ok[u] ? row : 0) * D;
#pragma unroll
                for (int j = 0; j < JMAX; ++j) {
                    const int c = lane * 4 + 256 * j;
                    v[u][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (c < D) v[u][j] = *reinterpret_cast<const f32x4*>(src + c);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < JMAX; ++j)
                    if (ok[u]) s[j] += v[u][j];
        }
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int c = lane * 4 + 256 * j;
            if (c < D) {
                if (dst >= 0) *reinterpret_cast<bf16x4*>((bf16_t*)a.d_ctx_feats + (long)dst * D + c) = to_bf16x4(s[j]);
                else mt[j] += s[j];
            }
        }
    }
    if (!a.d_mask_token) return;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int c = lane * 4 + 256 * j;
        if (c < D) *reinterpret_cast<f32x4*>(&macc_dyn[wave * D + c]) = mt[j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += 256) {
        const float v = fold4(macc_dyn + c, D);
        if (a.partials) a.partials[(long)blockIdx.x * D + c] = v;
        else atomicAdd(a.d_mask_token + c, v);
    }
}

// dst[m] = inv[m] >= 0 ? src[inv[m]] : 0     (gradient of the mask gather, jepa.py:399; inv == NULL: identity)
__global__ __launch_bounds__(256) void unmask_rows_kernel(wj_unmask_rows_args a) {
    for_each_row_col(a.M, a.D / 4, [&](int m, int c4) {
        const int c = c4 * 4;
        const int src = a.inv ? a.inv[m] : m;
        f32x4 y = f32x4{0.f, 0.f, 0.f, 0.f};
        if (src >= 0) {
            if (a.src_is_f32) y = *reinterpret_cast<const f32x4*>((const float*)a.src + (long)src * a.D + c);
            else y = to_f32x4(*reinterpret_cast<const bf16x4*>((const bf16_t*)a.src + (long)src * a.D + c));
        }
        if (a.dst_is_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.dst + (long)m * a.D + c) = to_bf16x4(y);
        else *reinterpret_cast<f32x4*>((float*)a.dst + (long)m * a.D + c) = y;
    });
}

// ------------------------------------------------------------------------------------------- teacher targets
__global__ __launch_bounds__(1024) void instnorm_kernel(wj_instnorm_args a) {
    __shared__ float red[16];
    const long base = (long)blockIdx.x * a.TD;
    const int n4 = a.TD / 4;
    const auto x = [&](int i) { return *reinterpret_cast<const f32x4*>(a.x + base + i * 4); };
    float mean;
    const float var = mean_sqdev(n4, (float)a.TD, x, red, mean) / (float)a.TD;
    const float k = rsqrtf(var + a.eps) * a.scale;
    float* t = a.targets + base;
    for (int i = threadIdx.x; i < n4; i += 1024) {
        f32x4 o = (x(i) - mean) * k;
        if (a.accumulate) o += *reinterpret_cast<const f32x4*>(t + i * 4);
        *reinterpret_cast<f32x4*>(t + i * 4) = o;
    }
}

// one pass over the K kept layer outputs: block = 1024 x float4 of one sample
__global__ __launch_bounds__(256) void instnorm_mean_kernel(wj_instnorm_mean_args a) {
    const int b = blockIdx.y;
    const float* xs[8] = {a.x0, a.x1, a.x2, a.x3, a.x4, a.x5, a.x6, a.x7};
    const float invn = 1.0f / (float)a.TD, invk = 1.0f / (float)a.K;
    float mu[8], sc[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        mu[l] = sc[l] = 0.f;
        if (l < a.K) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int p = 0; p < WJ_GROUP_STATS_SPLIT; ++p) {       // fixed order: bit-reproducible targets
                s1 += a.stats[(((long)l * a.B + b) * WJ_GROUP_STATS_SPLIT + p) * 2];
                s2 += a.stats[(((long)l * a.B + b) * WJ_GROUP_STATS_SPLIT + p) * 2 + 1];
            }
            mu[l] = s1 * invn;
            sc[l] = rsqrtf(fmaxf(s2 * invn - mu[l] * mu[l], 0.f) + a.eps) * invk;
        }
    }
    const long base = (long)b * a.TD;
    const int n4 = a.TD / 4;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) {
        f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            if (l < a.K) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xs[l] + base + i * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fmaf(v[e] - mu[l], sc[l], o[e]);
            }
        }
        *reinterpret_cast<f32x4*>(a.targets + base + i * 4) = o;
    }
}

// ------------------------------------------------------------------------------------------- masked MSE
__global__ __launch_bounds__(1024) void mse_count_kernel(const uint8_t* __restrict__ tgt, float* __restrict__ ws, long n) {
    __shared__ float red[16];
    // one workgroup, 16 mask bytes per load (a byte per load made this 88 us of pure latency); the count is an integer below
    // 2^24, so the float sum is exact in any order
    int k = 0;
    const bool vec = (reinterpret_cast<uintptr_t>(tgt) & 15) == 0;
    const long nv = vec ? n >> 4 : 0;
    for (long i = threadIdx.x; i < nv; i += 1024) {
        const uint4 v = reinterpret_cast<const uint4*>(tgt)[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t nz = (w[e] | (w[e] >> 1) | (w[e] >> 2) | (w[e] >> 3) | (w[e] >> 4) | (w[e] >> 5) | (w[e] >> 6) | (w[e] >> 7)) & 0x01010101u;
            k += __popc(nz);
        }
    }
    for (long i = (nv << 4) + threadIdx.x; i < n; i += 1024) k += tgt[i] ? 1 : 0;
    float c = block_sum((float)k, red);
    if (threadIdx.x == 0) ws[1] = c;
}

// One rows kernel for the whole loss family (include/wavjepa_hip.h: wj_loss_args), instantiated per kind.  d = fl32(bf16 pred - f32
// target); e(d) goes into the row sum, e'(d) * gk into dpreds.  gk carries MSE's factor 2 (its e' = 2 d), 1 for the other kinds;
// smooth-L1 multiplies by ib = fl32(1 / beta), formed once per thread.  sign(d) is exact: fl32(p - y) has the sign of p - y.
template <int KIND>
__device__ __forceinline__ void loss_elem(float d, float beta, float ib, float& e, float& g) {
    if constexpr (KIND == WJ_LOSS_MSE) {
        e = d * d;
        g = d;
    } else {
        const float ad = fabsf(d);
        const float sg = d > 0.f ? 1.0f : (d < 0.f ? -1.0f : 0.f);
        if constexpr (KIND == WJ_LOSS_L1) {
            e = ad;
            g = sg;
        } else if constexpr (KIND == WJ_LOSS_SMOOTH_L1) {
            const float q = d * ib;
            const bool quad = ad < beta;
            e = quad ? (0.5f * d) * q : ad - 0.5f * beta;
            g = quad ? q : sg;
        } else {                                   // WJ_LOSS_HUBER, beta is delta
            const bool quad = ad <= beta;
            e = quad ? (0.5f * d) * d : beta * (ad - 0.5f * beta);
            g = quad ? d : beta * sg;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void loss_rows_kernel(wj_loss_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D;
    const long R = a.rows ? (long)a.n_rows : (long)a.B * a.G * a.T;
    const float count = a.workspace[1];
    const float gk = (KIND == WJ_LOSS_MSE ? 2.0f : 1.0f) / ((float)D * (count + 1e-8f)) * a.gscale * (a.gscale_ptr ? a.gscale_ptr[0] : 1.0f);
    const float beta = a.beta, ib = KIND == WJ_LOSS_SMOOTH_L1 ? 1.0f / a.beta : 0.f;
    for (long r = blockIdx.x * 4L + wave; r < R; r += gridDim.x * 4L) {
        const long dense = a.rows ? (long)a.rows[r] : r;     // (b*G+g)*T + t; preds / dpreds are indexed by r
        const int t = (int)(dense % a.T);
        const long bg = dense / a.T;
        const int b = (int)(bg / a.G);
        const bool on = a.tgt[dense] != 0;
        float err = 0.f;
        for (int c = lane * 4; c < D; c += 256) {
            bf16x4 dp;
#pragma unroll
            for (int e = 0; e < 4; ++e) dp[e] = f2bf(0.f);
            if (on) {
                const bf16x4 p = *reinterpret_cast<const bf16x4*>((const bf16_t*)a.preds + r * D + c);
                const f32x4 y = *reinterpret_cast<const f32x4*>(a.targets + ((long)b * a.T + t) * D + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = bf2f(p[e]) - y[e];
                    float le, lg;
                    loss_elem<KIND>(d, beta, ib, le, lg);
                    err += le;
                    dp[e] = f2bf(lg * gk);
                }
            }
            if (a.dpreds) *reinterpret_cast<bf16x4*>((bf16_t*)a.dpreds + r * D + c) = dp;
        }
        err = wave_sum(err);
        if (lane == 0) a.workspace[2 + r] = on ? err / (float)D : 0.f;
    }
}

__global__ __launch_bounds__(1024) void mse_final_kernel(float* __restrict__ ws, float* __restrict__ loss, long R) {
    __shared__ float red[16];
    const float s = fold_partials(ws + 2, R, red);
    if (threadIdx.x == 0) {
        loss[0] = s / (ws[1] + 1e-8f);
        loss[1] = ws[1];
    }
}

// ------------------------------------------------------------------------------------------- EMA / AdamW / norms / casts
__global__ __launch_bounds__(256) void ema_kernel(wj_ema_args a) {
    const long n4 = a.n / 4;
    const float r = a.r, q = 1.0f - a.r;
    // (the plain loop, not for_each_flat: inside the walker's lambda the compiler contracts t * r + q * s around the other product -- other bits)
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(a.student + i * 4);
        f32x4 t = *reinterpret_cast<const f32x4*>(a.teacher + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = t[e] * r + q * s[e];
        *reinterpret_cast<f32x4*>(a.teacher + i * 4) = t;
        if (a.teacher_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.teacher_bf16 + i * 4) = to_bf16x4(t);
    }
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, float* __restrict__ ws, long n) {
    __shared__ float red[16];
    float s = 0.f;
    for_each_flat(n / 4, [&](long i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + i * 4);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    });
    s = block_sum(s, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void sumsq_final_kernel(const float* __restrict__ ws, float* __restrict__ out, int n, int accumulate) {
    __shared__ float red[16];
    const float s = fold_partials(ws, n, red);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s : s;
}

__global__ __launch_bounds__(256) void adamw_kernel(wj_adamw_args a) {
    const long n4 = a.n / 4;
    const float coef = adamw_clip_coef(a.sumsq, a.max_norm, a.grad_scale);
    float decay, step;
    adamw_rates(a.lr, a.weight_decay, a.bc1, decay, step);
    const float rbc2 = rsqrtf(a.bc2);
    // (the plain loop, as in ema_kernel: the moment updates are sums of two products; the element update is stream_pieces.h's
    // adamw_update4, shared with the grouped pass of csrc/optim.hip)
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 p = *reinterpret_cast<const f32x4*>(a.p + i * 4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.g + i * 4);
        if (a.zero_grad) *reinterpret_cast<f32x4*>(a.g + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 m = *reinterpret_cast<const f32x4*>(a.m + i * 4);
        f32x4 v = *reinterpret_cast<const f32x4*>(a.v + i * 4);
        adamw_update4(p, g, m, v, coef, decay, step, rbc2, a.beta1, a.beta2, a.eps);
        *reinterpret_cast<f32x4*>(a.p + i * 4) = p;
        *reinterpret_cast<f32x4*>(a.m + i * 4) = m;
        *reinterpret_cast<f32x4*>(a.v + i * 4) = v;
        if (a.p_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.p_bf16 + i * 4) = to_bf16x4(p);
    }
}

__global__ __launch_bounds__(256) void cast_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n) {
    const long n4 = n / 4;
    for_each_flat(n4, [&](long i) { *reinterpret_cast<bf16x4*>(dst + i * 4) = to_bf16x4(*reinterpret_cast<const f32x4*>(src + i * 4)); });
    for_each_flat(n - n4 * 4, [&](long i) { dst[n4 * 4 + i] = f2bf(src[n4 * 4 + i]); });      // the 1..3 elements behind the last whole group
}

// ------------------------------------------------------------------------------------------- batched bf16 transposes (W^T shadows)
// dst[off + c * rows + r] = src[off + r * cols + c] for every matrix of the table: the bf16 weight shadows of the transformer stacks,
// transposed once per step so that every dgrad dx = dy . W runs as a ROW-form GEMM against W^T (the persistent eight-phase kernel)
// instead of the col-form 256 x 128 schedule.  One workgroup per 64 x 64 tile: 16-byte reads along the source rows, a padded LDS
// tile (pitch 66 elements: the column walk of the transposed read touches 32 distinct banks), 16-byte writes along the destination
// rows.  table: int64 [n_mats][4] = (element offset, rows, cols, first tile of the matrix in the launch's tile list).
__global__ __launch_bounds__(256) void transpose_tiles_kernel(wj_transpose_args a) {
    __shared__ bf16_t tile[64][66];
    const int t = threadIdx.x;
    int q = 0;
#pragma unroll 1
    for (int x = 1; x < a.n_mats; ++x)
        if ((long)blockIdx.x >= a.table[4 * x + 3]) q = x;
    const long off = a.table[4 * q], rows = a.table[4 * q + 1], cols = a.table[4 * q + 2];
    const int local = (int)(blockIdx.x - a.table[4 * q + 3]);
    const int tiles_c = (int)(cols / 64);
    const int tr = local / tiles_c, tc = local - tr * tiles_c;
    const bf16_t* src = (const bf16_t*)a.src + off + (long)(tr * 64) * cols + tc * 64;
    bf16_t* dst = (bf16_t*)a.dst + off + (long)(tc * 64) * rows + tr * 64;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = (t >> 3) + 32 * u, c8 = (t & 7) * 8;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + (long)r * cols + c8);
#pragma unroll
        for (int x = 0; x < 8; ++x) tile[r][c8 + x] = v[x];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int c = (t >> 3) + 32 * u, r8 = (t & 7) * 8;       // destination row c (a source column), 8 source rows r8 ..
        bf16x8 v;
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = tile[r8 + x][c];
        *reinterpret_cast<bf16x8*>(dst + (long)c * rows + r8) = v;
    }
}

// ------------------------------------------------------------------------------------------- crop + normalise
__global__ __launch_bounds__(1024) void crop_kernel(wj_crop_args a) {
    __shared__ float red[16];
    const int bs = blockIdx.x, b = bs / a.S;
    const int start = a.starts[bs];
    const long n = (long)a.C * a.length;
    const float* src = a.src + (long)b * a.C * a.L_full;
    const auto x = [&](long i) {       // element i of the crop: channel c, sample start + l
        const int c = (int)(i / a.length), l = (int)(i - (long)c * a.length);
        return src[(long)c * a.L_full + start + l];
    };
    float mean;
    const float stdv = sqrtf(mean_sqdev(n, (float)n, x, red, mean) / (float)(n - 1));
    const float inv = 1.0f / (stdv + 1e-5f);
    const int orow = a.perm_inv ? a.perm_inv[bs] : bs;
    bf16_t* out = (bf16_t*)a.out + (long)orow * n;
    for (long i = threadIdx.x; i < n; i += 1024) out[i] = f2bf((x(i) - mean) * inv);
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int wj_gelu_bwd_bf16(const wj_gelu_bwd_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (a && a->rows) {
        if (!a->dpost || !a->pre || !a->dpre || a->n_rows < 0 || a->row_elems <= 0 || (a->row_elems & 7)) return WJ_ERR_ARG;
        if (a->n_rows == 0) return WJ_OK;
        hipLaunchKernelGGL(gelu_bwd_rows_kernel, dim3(grid_for((long)a->n_rows * (a->row_elems / 8), 256)), dim3(256), 0, STREAM,
                           (bf16_t*)a->dpost, (const bf16_t*)a->pre, (bf16_t*)a->dpre, a->rows, a->n_rows, a->row_elems / 8,
                           a->clear_dpost);
        return entry.launched();
    }
    if (!a || !a->dpost || !a->pre || !a->dpre || a->n <= 0 || (a->n & 7)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(grid_for(a->n / 8, 256)), dim3(256), 0, STREAM, (const bf16_t*)a->dpost,
                       (const bf16_t*)a->pre, (bf16_t*)a->dpre, (long)(a->n / 8));
    return entry.launched();
}

__global__ void spin_kernel(long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    while ((long)(__builtin_amdgcn_s_memtime() - t0) < ticks) __builtin_amdgcn_s_sleep(8);
}

extern "C" int wj_spin(const wj_spin_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || a->ticks < 0 || a->ticks > (1LL << 32)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, STREAM, (long)a->ticks);
    return entry.launched();
}

#ifdef WJ_LAB
// the footprint of a collective on its GPU (see the header): `passes` in-place read + rewrite sweeps by a few resident workgroups,
// stretched to `min_ticks` of the 100 MHz clock by pacing every piece
typedef __attribute__((ext_vector_type(4))) unsigned cf_u32x4;
__global__ __launch_bounds__(512) void collective_footprint_kernel(cf_u32x4* __restrict__ buf, long n16, long min_ticks, int passes) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const long per = (n16 + gridDim.x - 1) / gridDim.x;
    const long lo = per * blockIdx.x, hi = min(n16, lo + per);
    constexpr long PIECE = 512 * 8;                        // 64 KiB per workgroup and piece
    const long npieces = ((hi > lo ? hi - lo : 0) + PIECE - 1) / PIECE * passes;
    long done = 0;
    for (int ps = 0; ps < passes; ++ps)
        for (long p0 = lo; p0 < hi; p0 += PIECE) {
            cf_u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = p0 + u * 512 + threadIdx.x;
                v[u] = cf_u32x4{0u, 0u, 0u, 0u};
                if (i < hi) v[u] = __builtin_nontemporal_load(buf + i);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long i = p0 + u * 512 + threadIdx.x;
                asm volatile("" : "+v"(v[u].x));           // (keeps the rewrite of an unchanged value from being dropped)
                if (i < hi) __builtin_nontemporal_store(v[u], buf + i);
            }
            ++done;
            if (min_ticks > 0) {
                const unsigned long long due = (unsigned long long)(min_ticks * done / npieces);
                while (__builtin_amdgcn_s_memrealtime() - t0 < due) __builtin_amdgcn_s_sleep(16);
            }
        }
}

extern "C" int wj_collective_footprint(const wj_collective_footprint_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->buf || a->bytes <= 0 || (a->bytes & 15) || ((uintptr_t)a->buf & 15) || a->workgroups < 1 || a->workgroups > 256 ||
        a->passes < 1 || a->passes > 8 || a->min_ticks < 0)
        return WJ_ERR_ARG;
    hipLaunchKernelGGL(collective_footprint_kernel, dim3(a->workgroups), dim3(512), 0, STREAM, (cf_u32x4*)a->buf, (long)(a->bytes / 16),
                       (long)a->min_ticks, a->passes);
    return entry.launched();
}
#endif

extern "C" int wj_zero_rows(const wj_zero_rows_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->buf || !a->rows || a->n_rows < 0 || a->row_bytes <= 0 || (a->row_bytes & 15)) return WJ_ERR_ARG;
    if (a->n_rows == 0) return WJ_OK;
    hipLaunchKernelGGL(zero_rows_kernel, dim3(grid_for((long)a->n_rows * (a->row_bytes / 16), 256)), dim3(256), 0, STREAM,
                       (char*)a->buf, a->rows, a->n_rows, a->row_bytes / 16);
    return entry.launched();
}

extern "C" int wj_conv_weight_layout(const wj_conv_w_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->src || !a->dst || a->C_out <= 0 || a->C_in <= 0 || a->k <= 0 || a->mode < 0 || a->mode > 2) return WJ_ERR_ARG;
    if (a->mode == 1 && (a->U <= 0 || a->rho < 0 || a->rho + a->stride * (a->U - 1) >= a->k)) return WJ_ERR_ARG;
    const long n = a->mode == 1 ? (long)a->U * a->C_out * a->C_in : (long)a->C_out * a->C_in * a->k;
    hipLaunchKernelGGL(conv_w_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_add_pos(const wj_add_pos_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->x || !a->pos || a->M <= 0 || a->T <= 0 || a->D <= 0 || (a->D & 3)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(add_pos_kernel, dim3(grid_for((long)a->M * a->D / 4, 256)), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_mask_gather_rows(const wj_gather_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->x || !a->idx || !a->out || a->n_rows < 0 || a->D <= 0) return WJ_ERR_ARG;
    if (a->elem_bytes != 2 && a->elem_bytes != 4) return WJ_ERR_ARG;
    const int row_bytes = a->D * a->elem_bytes;
    if (row_bytes & 15) return WJ_ERR_ARG;
    if (a->n_rows == 0) return WJ_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(a->n_rows, 1, 16384)), dim3(256), 0, STREAM, (const char*)a->x, a->idx,
                       (char*)a->out, a->n_rows, row_bytes);
    return entry.launched();
}

extern "C" int wj_mask_scatter_fill_pos(const wj_scatter_fill_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->ctx_feats || !a->inv || !a->mask_token || !a->pos || a->B <= 0 || a->T <= 0 || a->D <= 0 || (a->D & 3) ||
        a->G <= 0)
        return WJ_ERR_ARG;
    if (a->rows) {
        if (a->n_rows < 0) return WJ_ERR_ARG;
        if (a->n_rows == 0) return WJ_OK;
        hipLaunchKernelGGL(scatter_fill_rows_kernel, dim3(grid_for((long)a->n_rows, 4)), dim3(256), 0, STREAM, *a);
        return entry.launched();
    }
    hipLaunchKernelGGL(scatter_fill_kernel, dim3(grid_for((long)a->B * a->T, 4)), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_scatter_fill_bwd_partial_rows(int B, int T) { return (int)(((long)B * T + SFB_ROWS - 1) / SFB_ROWS); }
// `partials`: one row of D floats per workgroup
int64_t wj_scatter_fill_bwd_ws_bytes(const wj_scatter_fill_bwd_args* a) { return (int64_t)wj_scatter_fill_bwd_partial_rows(a->B, a->T) * a->D * 4; }

extern "C" int wj_mask_scatter_fill_pos_bwd(const wj_scatter_fill_bwd_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->d_in || !a->inv || !a->d_ctx_feats || a->B <= 0 || a->T <= 0 || a->D <= 0 || (a->D & 3) || a->D > 1024 ||
        a->G <= 0 || a->G > 15)              // (a wave's 4 rows x (G + 1) indices are fetched by one load per lane)
        return WJ_ERR_ARG;
    const int grid = wj_scatter_fill_bwd_partial_rows(a->B, a->T);
    if (a->D <= 512) hipLaunchKernelGGL(scatter_fill_bwd_kernel<2>, dim3(grid), dim3(256), (size_t)4 * a->D * sizeof(float), STREAM, *a);
    else hipLaunchKernelGGL(scatter_fill_bwd_kernel<4>, dim3(grid), dim3(256), (size_t)4 * a->D * sizeof(float), STREAM, *a);
    return entry.launched();
}

extern "C" int wj_unmask_rows_f32(const wj_unmask_rows_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->src || !a->dst || a->M <= 0 || a->D <= 0 || (a->D & 3)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(unmask_rows_kernel, dim3(grid_for((long)a->M * a->D / 4, 256)), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_instnorm_accumulate(const wj_instnorm_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->x || !a->targets || a->B <= 0 || a->TD <= 0 || (a->TD & 3)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(instnorm_kernel, dim3(a->B), dim3(1024), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_instnorm_mean(const wj_instnorm_mean_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->stats || !a->targets || a->B <= 0 || a->TD <= 0 || (a->TD & 3) || a->K < 1 || a->K > 8) return WJ_ERR_ARG;
    const float* xs[8] = {a->x0, a->x1, a->x2, a->x3, a->x4, a->x5, a->x6, a->x7};
    for (int l = 0; l < a->K; ++l)
        if (!xs[l]) return WJ_ERR_ARG;
    hipLaunchKernelGGL(instnorm_mean_kernel, dim3(grid_for(a->TD / 4, 256, 32), a->B), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

// count -> rows<kind> -> final: one launch sequence for wj_masked_mse (kind MSE) and wj_masked_loss; validation precedes every launch
static int masked_loss_launch(const wj_loss_args* a, void* stream, const CheckedEntry& entry) {
    if (!a->preds || !a->targets || !a->tgt || !a->loss || !a->workspace) return WJ_ERR_ARG;
    if (a->B <= 0 || a->G <= 0 || a->T <= 0 || a->D <= 0 || (a->D & 3)) return WJ_ERR_ARG;
    const long Rd = (long)a->B * a->G * a->T;          // dense positions (the target count runs over all of them)
    if (a->rows && a->n_rows < 0) return WJ_ERR_ARG;
    if (a->kind < WJ_LOSS_MSE || a->kind > WJ_LOSS_HUBER) return WJ_ERR_UNSUPPORTED;
    if ((a->kind == WJ_LOSS_SMOOTH_L1 || a->kind == WJ_LOSS_HUBER) && !(a->beta > 0.f && a->beta <= 3.402823466e38f)) return WJ_ERR_ARG;   // NaN, inf, <= 0
    const long R = a->rows ? (long)a->n_rows : Rd;    // rows actually held by preds / dpreds
    hipLaunchKernelGGL(mse_count_kernel, dim3(1), dim3(1024), 0, STREAM, a->tgt, a->workspace, Rd);
    if (R > 0) {
        const dim3 grid(grid_for(R, 4));
        switch (a->kind) {
            case WJ_LOSS_MSE: hipLaunchKernelGGL(loss_rows_kernel<WJ_LOSS_MSE>, grid, dim3(256), 0, STREAM, *a); break;
            case WJ_LOSS_L1: hipLaunchKernelGGL(loss_rows_kernel<WJ_LOSS_L1>, grid, dim3(256), 0, STREAM, *a); break;
            case WJ_LOSS_SMOOTH_L1: hipLaunchKernelGGL(loss_rows_kernel<WJ_LOSS_SMOOTH_L1>, grid, dim3(256), 0, STREAM, *a); break;
            default: hipLaunchKernelGGL(loss_rows_kernel<WJ_LOSS_HUBER>, grid, dim3(256), 0, STREAM, *a); break;
        }
    }
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(1024), 0, STREAM, a->workspace, a->loss, R);
    return entry.launched();
}

// workspace of both entries: the target count and the loss sum, then one partial per dense position
static int64_t masked_loss_ws_bytes(int B, int G, int T) { return (2 + (int64_t)B * G * T) * 4; }
int64_t wj_masked_mse_ws_bytes(const wj_mse_args* a) { return masked_loss_ws_bytes(a->B, a->G, a->T); }
int64_t wj_masked_loss_ws_bytes(const wj_loss_args* a) { return masked_loss_ws_bytes(a->B, a->G, a->T); }

extern "C" int wj_masked_mse(const wj_mse_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a) return WJ_ERR_ARG;
    const wj_loss_args l = {a->preds, a->targets, a->tgt, a->rows, a->loss, a->dpreds, a->workspace, a->gscale_ptr,
                            a->B, a->G, a->T, a->D, a->n_rows, a->gscale, WJ_LOSS_MSE, 0.f};
    return masked_loss_launch(&l, stream, entry);
}

extern "C" int wj_masked_loss(const wj_loss_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a) return WJ_ERR_ARG;
    return masked_loss_launch(a, stream, entry);
}

extern "C" int wj_ema_update(const wj_ema_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->student || !a->teacher || a->n <= 0 || (a->n & 3)) return WJ_ERR_ARG;
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(a->n / 4, 256)), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

constexpr int SUMSQ_MAX_GRID = 1024;           // one partial float per workgroup in the workspace
int64_t wj_grad_sumsq_ws_bytes(const wj_sumsq_args*) { return SUMSQ_MAX_GRID * 4; }

extern "C" int wj_grad_sumsq(const wj_sumsq_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->g || !a->out || !a->workspace || a->n <= 0 || (a->n & 3)) return WJ_ERR_ARG;
    int grid = grid_for(a->n / 4, 256, SUMSQ_MAX_GRID);
    if (a->workgroups > 0 && a->workgroups < grid) grid = a->workgroups;
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(256), 0, STREAM, a->g, a->workspace, (long)a->n);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(1024), 0, STREAM, (const float*)a->workspace, a->out, grid, a->accumulate);
    return entry.launched();
}

extern "C" int wj_adamw_step(const wj_adamw_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->p || !a->g || !a->m || !a->v || a->n <= 0 || (a->n & 3)) return WJ_ERR_ARG;
    int grid = grid_for(a->n / 4, 256);
    if (a->workgroups > 0 && a->workgroups < grid) grid = a->workgroups;
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_transpose_bf16(const wj_transpose_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->src || !a->dst || !a->table || a->n_mats <= 0 || a->n_tiles <= 0) return WJ_ERR_ARG;
    if (((uintptr_t)a->src | (uintptr_t)a->dst) & 15) return WJ_ERR_ARG;
    hipLaunchKernelGGL(transpose_tiles_kernel, dim3(a->n_tiles), dim3(256), 0, STREAM, *a);
    return entry.launched();
}

extern "C" int wj_cast_f32_to_bf16(const wj_cast_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->src || !a->dst || a->n <= 0) return WJ_ERR_ARG;
    hipLaunchKernelGGL(cast_kernel, dim3(grid_for(a->n / 4 + 1, 256)), dim3(256), 0, STREAM, a->src, (bf16_t*)a->dst, (long)a->n);
    return entry.launched();
}

extern "C" int wj_crop_normalize_bf16(const wj_crop_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->src || !a->starts || !a->out || a->B <= 0 || a->S <= 0 || a->C <= 0 || a->length <= 1 || a->L_full < a->length)
        return WJ_ERR_ARG;
    hipLaunchKernelGGL(crop_kernel, dim3(a->B * a->S), dim3(1024), 0, STREAM, *a);
    return entry.launched();
}
