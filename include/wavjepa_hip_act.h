/* C ABI of libwavjepa_hip_act.so: the forward GEMM of a feed-forward block's linear1 with the activation chosen per call, built from
 * the GEMM sources of libwavjepa_hip.so (csrc/gemm.hip, csrc/gemm_persist.hip with -DWJ_ACT_LIB) into a library of its own:
 * libwavjepa_hip.so, its header, its ABI version and its entry table are exactly what they were.  Same conventions: the entry is
 * `int entry(const ARGS*, void* stream)`, 0 or a negative WJ_ERR code answered before any launch; the two query entries at the end
 * mirror wj_struct_size / wj_workspace_bytes for the struct and entry declared here (entry table: csrc/abi_table.h). */
#ifndef WAVJEPA_HIP_ACT_H
#define WAVJEPA_HIP_ACT_H
#include "wavjepa_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The activation act of nn.TransformerEncoderLayer(activation = ...), as torch computes it on a bf16 tensor:
 *   WJ_ACT_GELU       nn.GELU():                   0.5 h (1 + erf(h / sqrt 2))                       -- what wj_gemm_bf16 computes
 *   WJ_ACT_RELU       nn.ReLU():                   max(h, 0);             act' = 1 if h > 0 else 0 (0 at h == 0)
 *   WJ_ACT_GELU_TANH  nn.GELU(approximate="tanh"): 0.5 h (1 + tanh(c (h + 0.044715 h^3))), c = sqrt(2 / pi)
 *   WJ_ACT_SILU       nn.SiLU():                   h s, s = 1 / (1 + exp(-h));   act' = s (1 + h (1 - s)) */
enum { WJ_ACT_GELU = 0, WJ_ACT_RELU, WJ_ACT_GELU_TANH, WJ_ACT_SILU };

/* wj_gemm_bf16 with the activation of its two forward GELU forms replaced by `act`; every other field means what it means there.
 *   gemm.epilogue = WJ_EPI_BIAS_GELU2: C = act'(h), C2 = act(h);   WJ_EPI_BIAS_GELU: C = act(h)      (any other: WJ_ERR_ARG)
 * Rounding points as the GELU forms: h = bf16(acc + bias); act and act' in fp32 from that bf16 value, each rounded to bf16 once.
 * Every finite bf16 h gives finite outputs; where act' has saturated it is exactly 1 or (+-)0.  The backward needs no entry of its
 * own: WJ_EPI_MUL_GELU_GRAD multiplies by the stored act' tile whatever produced it.
 *   act outside the enum: WJ_ERR_ARG.
 *   Row-form operands only (a_trans = b_trans = 0; else WJ_ERR_UNSUPPORTED), in the schedules linear1 reaches: the 256 x 128 tile
 *   (variant 0), the eight-phase 256 x 256 tile (3) and the persistent kernel (4), picked from the shape as wj_gemm_bf16 picks them or
 *   forced through gemm.schedule.  Forcing another one (schedule 2, 3: the plain / ping-pong 256 x 256 tiles; 6, 7: row panels and the
 *   deferred epilogue): WJ_ERR_UNSUPPORTED.
 *   act = WJ_ACT_GELU runs the instantiations wj_gemm_bf16 runs for the same arguments: the same bits. */
typedef struct {
    wj_gemm_args gemm;
    int32_t act;
} wj_gemm_act_args;
int wj_gemm_bf16_act(const wj_gemm_act_args*, void* stream);

/* sizeof of a struct declared in this header by name (-1: unknown); scratch bytes of an entry declared here for the dimensions in
 * args (pointers ignored; -1: unknown entry) */
int wj_act_struct_size(const char* name);
int64_t wj_act_workspace_bytes(const char* fn, const void* args);

#ifdef __cplusplus
}
#endif
#endif /* WAVJEPA_HIP_ACT_H */
