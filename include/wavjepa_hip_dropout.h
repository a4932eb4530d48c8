/* C ABI of libwavjepa_hip_dropout.so: the dropout forms of three kernel families of libwavjepa_hip.so (header wavjepa_hip.h), built
 * from the same sources (csrc/norm.hip, csrc/attention_stream.hip with -DWJ_DROPOUT_LIB, csrc/dropout.hip) into a library of their own:
 * libwavjepa_hip.so, its header, its ABI version and its entry table are exactly what they were.  Same conventions: every entry is
 * `int entry(const ARGS*, void* stream)`, 0 or a negative WJ_ERR code answered before any launch; the two query entries at the end
 * mirror wj_struct_size / wj_workspace_bytes for the structs and entries declared here (entry table: csrc/abi_table.h). */
#ifndef WAVJEPA_HIP_DROPOUT_H
#define WAVJEPA_HIP_DROPOUT_H
#include "wavjepa_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------
 * Dropout (training mode of nn.TransformerEncoderLayer(dropout = p, norm_first = False)): the entries of libwavjepa_hip_dropout.so.
 * New entries with new argument structs, each the parent entry's struct (wavjepa_hip.h) followed by the shared tail below.
 * The masks come from a counter-based generator (Philox4x32-10, csrc/dropout_pieces.h, which also documents the grouping of eight
 * draws per call at every site): a mask is a pure function of (seed, call, stream_id, element), nothing about it is stored, and the
 * backward / the second forward of recompute mode regenerate it from the same tail.
 *   seed      : 64-bit key (the host mixes the data-parallel rank in)
 *   call      : step counter (JEPA.global_step)
 *   stream_id : site | layer << 8 | stack << 16   (site 1 attention probabilities, 2 dropout1, 3 FFN, 4 dropout2)
 *   p         : in [0, 1) (outside: WJ_ERR_ARG).  thr = round(p * 65536) (at most 65535); an element is kept iff its 16-bit draw >= thr
 *               and the survivors are scaled by 65536 / (65536 - thr) in fp32, the scale of the rate actually drawn.
 * -----------------------------------------------------------------------------------------------------------*/
typedef struct {
    uint64_t seed;
    uint32_t call;
    uint32_t stream_id;
    float p;
} wj_dropout_args;

/* In place over one or two bf16 [M][N] tensors (x2 optional) with the SAME mask: x <- bf16(float(x) * scale) where kept, +0 where
 * dropped.  N % 8 == 0 (16-byte accesses, one generator call each); element (row, col): group row * N / 8 + col / 8, draw col % 8.
 * The engine runs it over linear1's two outputs (gelu and gelu') behind the BIAS_GELU2 GEMM. */
typedef struct {
    void* x;
    void* x2;
    int64_t ldx; /* row stride of both, in elements (a multiple of 8) */
    int32_t M, N;
    wj_dropout_args drop;
} wj_dropout_rows_args;
int wj_dropout_rows(const wj_dropout_rows_args*, void* stream);

/* wj_layernorm_fwd with dropout on the addend: s = x + r o m * scale (r required, D % 8 == 0; no lean form, no fp8 output).
 * Element (m, col) of r: group m * D / 8 + col / 8, draw col % 8. */
typedef struct {
    wj_ln_fwd_args ln;
    wj_dropout_args drop;
} wj_ln_fwd_drop_args;
int wj_layernorm_fwd_drop(const wj_ln_fwd_drop_args*, void* stream);
/* wj_layernorm_bwd of the above: x-hat from s = x + r o m * scale; ds_f32 unchanged (the residual's gradient); ds_bf16 =
 * bf16(ds o m * scale), exactly 0 where dropped; dbias = column sums of that masked bf16 tensor.  r required, D % 8 == 0. */
typedef struct {
    wj_ln_bwd_args ln;
    wj_dropout_args drop;
} wj_ln_bwd_drop_args;
int wj_layernorm_bwd_drop(const wj_ln_bwd_drop_args*, void* stream);

/* wj_attn_stream_fwd / _bwd with dropout on the probabilities: O = (softmax(S) o m * scale) V.  The dropped elements of the bf16 P are
 * zeroed in front of the P.V MFMA and the scale is applied once to O in fp32, so P's rounding point and lse are the parent's.
 * Backward: dV += (P o m)^T dO * scale, dP = (dO V^T) o m * scale, dS = P o (dP - delta) with delta = rowsum(dO o O) of the dropped,
 * scaled O.  The mask is a function of (sequence of the launch, head, query, key) only.  Everything else as the parent entries
 * (hd in {32, 64}, 16: WJ_ERR_UNSUPPORTED; T <= 1024). */
typedef struct {
    wj_attn_fwd_args attn;
    wj_dropout_args drop;
} wj_attn_fwd_drop_args;
int wj_attn_stream_fwd_drop(const wj_attn_fwd_drop_args*, void* stream);
typedef struct {
    wj_attn_bwd_args attn;
    wj_dropout_args drop;
} wj_attn_bwd_drop_args;
int wj_attn_stream_bwd_drop(const wj_attn_bwd_drop_args*, void* stream);

/* sizeof of a struct declared in this header by name (-1: unknown); scratch bytes of an entry declared here for the dimensions in
 * args (pointers ignored; -1: unknown entry) */
int wj_dropout_struct_size(const char* name);
int64_t wj_dropout_workspace_bytes(const char* fn, const void* args);

#ifdef __cplusplus
}
#endif
#endif /* WAVJEPA_HIP_DROPOUT_H */
