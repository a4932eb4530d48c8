// wj_dropout_rows: dropout in place over one or two bf16 [M][N] tensors with the same mask (the FFN site: linear1's gelu and gelu'
// outputs behind the BIAS_GELU2 GEMM), and the host side of the shared tail wj_dropout_args.  HBM-bound: one 16-byte access = eight
// elements = one generator call (csrc/dropout_pieces.h) per thread and iteration.  The library's two query entries are at the end.
#include "common.h"
#include "dropout_host.h"
#include "abi_queries.h"

namespace {

__device__ __forceinline__ bf16x8 drop8(bf16x8 v, uint32_t keep, float scale) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (keep >> e) & 1u ? f2bf(bf2f(v[e]) * scale) : f2bf(0.f);
    return v;
}

__global__ __launch_bounds__(256) void dropout_rows_kernel(bf16_t* __restrict__ x, bf16_t* __restrict__ x2, long ldx, int M, int N, DropParams d) {
    const int gpr = N >> 3;                                   // groups per row
    const long total = (long)M * gpr;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long row = idx / gpr;
        const int cg = (int)(idx - row * gpr);
        const uint32_t keep = drop_keep_bits(d, (uint64_t)idx);   // group = row * N / 8 + col / 8
        bf16x8* p = reinterpret_cast<bf16x8*>(x + row * ldx + cg * 8);
        *p = drop8(*p, keep, d.scale);
        if (x2) {
            bf16x8* p2 = reinterpret_cast<bf16x8*>(x2 + row * ldx + cg * 8);
            *p2 = drop8(*p2, keep, d.scale);
        }
    }
}

}  // namespace

extern "C" WJ_EXPORT int wj_dropout_rows(const wj_dropout_rows_args* a, void* stream) {
    WJ_CLEAR_STALE_ERROR();
    if (!a || !a->x || a->M <= 0 || a->N <= 0 || (a->N & 7) || (a->ldx & 7) || a->ldx < a->N) return WJ_ERR_ARG;
    if (((uintptr_t)a->x & 15) || ((uintptr_t)a->x2 & 15)) return WJ_ERR_ARG;
    DropParams d;
    if (!drop_params(a->drop, d)) return WJ_ERR_ARG;
    const long total = (long)a->M * (a->N >> 3);
    long grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (bf16_t*)a->x, (bf16_t*)a->x2, (long)a->ldx, a->M,
                       a->N, d);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

WJ_ABI_QUERIES(WJ_DROPOUT_ENTRIES, WJ_DROPOUT_OTHER_STRUCTS, wj_dropout_struct_size, wj_dropout_workspace_bytes)
