/* C ABI of libwavjepa_hip_monitor.so: the collapse monitor of the JEPA step (csrc/monitor.hip), in a library of its own so that
 * libwavjepa_hip.so, its header, its ABI version and its entry table are exactly what they were.  Same conventions as wavjepa_hip.h:
 * the entry is `int entry(const ARGS*, void* stream)`, 0 or a negative WJ_ERR code answered before any launch; the two query entries
 * at the end mirror wj_struct_size / wj_workspace_bytes for what is declared here (entry table: csrc/abi_table.h). */
#ifndef WAVJEPA_HIP_MONITOR_H
#define WAVJEPA_HIP_MONITOR_H
#include "wavjepa_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Masked moments: the spread of the predictions and of the teacher's targets over the rows the masked loss uses (data2vec's
 * compute_var).  The rows are the multiset of every (b, g, t) with tgt[b][g][t] != 0 -- a token that is a target in two groups counts
 * twice, as in the loss.  Per column c over the n rows: var_c = M2_c / (n - 1) (unbiased; n < 2 gives 0), and
 *   stat = mean_c sqrt(var_c + 1e-6)           ( = torch.sqrt(y.var(dim=0) + 1e-6).mean() on those rows )
 *   out[0] = stat of the preds (bf16), out[1] = stat of the targets (fp32, row targets[b][t]), out[2] = n, out[3] = 0 (reserved).
 * preds / targets / tgt / rows / B / G / T / D / n_rows are wj_mse_args' own: preds bf16 [B*G][T][D] (dense form) or the n_rows
 * packed rows (rows != NULL, row r standing for the dense index rows[r] = (b*G+g)*T + t), targets f32 [B][T][D], tgt u8 [B][G][T].
 * Every row is tested against tgt[rows[r]]: a ragged row list also holds visible context rows, which are no targets; the trimmed
 * list holds targets only.
 * col (optional): f64 [2][2][D], col[q][0][c] the mean and col[q][1][c] the centred sum of squares M2 of column c; q = 0 preds,
 * 1 targets.  With out[2] they are what a data-parallel run merges across ranks (Chan).
 * Two launches, no atomics, the same bits from two launches of the same input.  Pass 1: a workgroup streams WJ_MOMENTS_ROWS rows of
 * WJ_MOMENTS_COLS columns with 16-byte loads and leaves one record (count, mean, M2) in the workspace; every accumulator is fp64
 * and shifted by the first target value its thread saw, so a constant column has M2 exactly 0 and a mean far above the spread costs
 * nothing.  Pass 2: one workgroup merges the records in row order in fp64 and forms out and col.
 * workspace: f64, wj_monitor_workspace_bytes("wj_masked_moments", args) bytes, 8-byte aligned; preds and targets 16-byte aligned.
 * D % 8 != 0, or more than WJ_MOMENTS_MAX_GROUPS * WJ_MOMENTS_ROWS rows: WJ_ERR_UNSUPPORTED; bad sizes, NULL or misaligned required
 * pointers: WJ_ERR_ARG. */
#define WJ_MOMENTS_ROWS 1024
#define WJ_MOMENTS_COLS 64
#define WJ_MOMENTS_MAX_GROUPS 2048
typedef struct {
    const void* preds;
    const float* targets;
    const uint8_t* tgt;
    const int32_t* rows;     /* optional int32 [n_rows]: ragged / trimmed form */
    float* out;              /* f32 [4] */
    double* col;             /* optional f64 [2][2][D] */
    double* workspace;
    int32_t B, G, T, D;
    int32_t n_rows;
} wj_moments_args;
int wj_masked_moments(const wj_moments_args*, void* stream);

/* sizeof of a struct declared in this header by name (-1: unknown); scratch bytes of an entry declared here for the dimensions in
 * args (pointers ignored: the answer covers max(B*G*T, n_rows) rows, so one buffer serves all three row forms; -1: unknown entry
 * or dimensions it refuses) */
int wj_monitor_struct_size(const char* name);
int64_t wj_monitor_workspace_bytes(const char* fn, const void* args);

#ifdef __cplusplus
}
#endif
#endif /* WAVJEPA_HIP_MONITOR_H */
