// Internal seam between csrc/gemm.hip (variant selection, the C ABI entry) and the persistent schedules (csrc/gemm_persist.hip,
// csrc/gemm_pde.hip, csrc/gemm_panel.hip), and the host pieces they share.  Not part of the C ABI.  The device pieces: gemm_pieces.h.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include "common.h"
#include "../../include/wavjepa_hip.h"

// true when wj_gemm_persist_launch can run this problem (row-form operands, K % 128 == 0, >= 256 output tiles, a forward epilogue)
bool wj_gemm_persist_eligible(const wj_gemm_args* a);
// WJ_OK, or WJ_ERR_UNSUPPORTED (not eligible / no scheduling slot left for this stream: the caller takes another variant)
int wj_gemm_persist_launch(const wj_gemm_args* a, hipStream_t s);
// libwavjepa_hip_act.so (-DWJ_ACT_LIB) in its place: the two forward GELU forms with activation `act` (common.h: ACT_*)
int wj_gemm_persist_launch_act(const wj_gemm_args* a, int act, hipStream_t s);

// the stream's set of 8 tile counters (zero between launches), or NULL when no set is free; *dev_out = the current device
unsigned* wj_gemm_persist_counters(hipStream_t s, int* dev_out);
// resident workgroups per XCD for this call (wj_gemm_args.persist_cus, or the process default)
int wj_gemm_persist_wpx(const wj_gemm_args* a);

// csrc/gemm_pde.hip: the persistent kernel with a DEFERRED epilogue (variant 6: 128 x 256 items, the GELU of item i under the K loop of item
// i + 1); row-form operands, K % 128 == 0, K >= 256, N % 256 == 0, BIAS_GELU / BIAS_GELU2 / CONV_GELU
bool wj_gemm_pde_eligible(const wj_gemm_args* a);
int wj_gemm_pde_launch(const wj_gemm_args* a, hipStream_t s);

// csrc/gemm_panel.hip: the row-panel schedule for thin outputs (variant 5: N = 384, row-form operands, K % 128 == 0, K >= 256, WJ_EPI_BF16)
bool wj_gemm_panel_eligible(const wj_gemm_args* a);
int wj_gemm_panel_launch(const wj_gemm_args* a, hipStream_t s);

namespace {

// Launch KERN (512 threads) with `lds` bytes of dynamic LDS.  Above 64 KiB a kernel has to be allowed its LDS once per device
// (hipFuncAttributeMaxDynamicSharedMemorySize); KERN is a template argument so that every kernel has its own flags.
template <auto KERN, class... Args>
int launch_with_lds(dim3 grid, int lds, hipStream_t s, Args... args) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return WJ_ERR_LAUNCH;
    static std::atomic<bool> lds_ok[32];
    if (!lds_ok[dev].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return WJ_ERR_LAUNCH;
        lds_ok[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(KERN, grid, dim3(512), lds, s, args...);
    WJ_CHECK_LAUNCH();
    return WJ_OK;
}

// The operands of a row-form call as the persistent kernels take them: byte pointers, leading dimensions in bytes, the segment rule of
// CONV_GELU with its "every row valid" default.  PArgs / DArgs / QArgs start with it.
struct RowArgs {
    const char* A;
    const char* B;
    char* C;
    char* C2;
    const float* bias;
    long ldc_b;
    unsigned lda_b, ldb_b;
    int M, N, K;
    int seg_rows, seg_valid;
    void set(const wj_gemm_args* a) {
        A = (const char*)a->A; B = (const char*)a->B; C = (char*)a->C; C2 = (char*)a->C2; bias = (const float*)a->bias;
        ldc_b = a->ldc * 2; lda_b = (unsigned)(a->lda * 2); ldb_b = (unsigned)(a->ldb * 2);
        M = a->M; N = a->N; K = a->K;
        seg_rows = a->seg_rows > 0 ? a->seg_rows : 1;
        seg_valid = a->seg_rows > 0 ? a->seg_valid : 1;
    }
};

// What every persistent schedule asks of a call: row-form dense operands, one K slice, 16-byte LDS-DMA / vector stores at every tile
// origin, and 32-bit per-lane offsets inside a work item of rows_a rows of A and rows_b rows of B.  The shape rules are each kernel's own.
inline bool row_form_common_ok(const wj_gemm_args* a, int rows_a, int rows_b) {
    if (a->a_trans || a->b_trans || a->rowmap || a->split_k > 1) return false;
    if ((a->lda & 7) || (a->ldb & 7) || (a->ldc & 7)) return false;
    if (((uintptr_t)a->A | (uintptr_t)a->B | (uintptr_t)a->C | (uintptr_t)a->bias) & 15) return false;
    if (a->lda * 2 * rows_a >= (1l << 31) || a->ldb * 2 * rows_b >= (1l << 31)) return false;
    return true;
}

}  // namespace
