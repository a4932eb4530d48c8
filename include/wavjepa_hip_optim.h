/* C ABI of libwavjepa_hip_optim.so: the AdamW pass with parameter groups (csrc/optim.hip), in a library of its own so that
 * libwavjepa_hip.so, its header, its ABI version and its entry table are exactly what they were.  Same conventions as wavjepa_hip.h:
 * the entry is `int entry(const ARGS*, void* stream)`, 0 or a negative WJ_ERR code answered before any launch; the two query entries
 * at the end mirror wj_struct_size / wj_workspace_bytes for what is declared here (entry table: csrc/abi_table.h). */
#ifndef WAVJEPA_HIP_OPTIM_H
#define WAVJEPA_HIP_OPTIM_H
#include "wavjepa_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* wj_adamw_step with a learning rate and a weight decay per parameter group.  Every element belongs to one of n_groups groups; the
 * arithmetic per element is wj_adamw_step's own (one copy: adamw_rates / adamw_update4 of csrc/stream_pieces.h) with the group's pair:
 *   decay = 1 - lr[k] * weight_decay[k];   step = lr[k] / bc1;   p *= decay;  m, v as there;  p -= step * m / (sqrt(v) * rsqrt(bc2) + eps)
 * The clip coefficient is wj_adamw_step's, from the ONE global sumsq: clipping is over all parameters, as clip_grad_norm_ is.
 * An element of a group k is bit-equal to wj_adamw_step run with lr[k] / weight_decay[k] on the same buffers.
 * group_map: DEVICE pointer, one byte per granule of WJ_ADAMW_GRANULE = 8 elements of the whole flat buffer (a slot of the flat layout
 * starts on a granule and its padding belongs to it), the group index of the granule, < n_groups.  It is static: built once, read by
 * every launch.  first: the index IN THE FLAT BUFFER of the launch's first element (p, g, m, v, p_bf16 point AT that element, as for
 * wj_adamw_step on a sub-range); element i of the launch reads group_map[(first + i) / 8].  lr / weight_decay travel by value: they
 * change every step (schedules) and no upload is wanted.  A map byte >= n_groups is the caller's error; the kernel reads its table
 * entry modulo WJ_ADAMW_MAX_GROUPS, so it never indexes outside the table.
 * n % 8 != 0, first % 8 != 0, n <= 0, first < 0, n_groups outside 1 .. WJ_ADAMW_MAX_GROUPS, NULL p / g / m / v / group_map, or p / g /
 * m / v not 16-byte (p_bf16: 8-byte) aligned: WJ_ERR_ARG before any launch.  The remaining fields are wj_adamw_args' own. */
#define WJ_ADAMW_MAX_GROUPS 64
#define WJ_ADAMW_GRANULE 8
typedef struct {
    float* p;
    float* g;            /* read; with zero_grad also cleared */
    float* m;
    float* v;
    void* p_bf16;
    const float* sumsq;
    int64_t n;
    float beta1, beta2, eps, bc1, bc2, max_norm, grad_scale;
    int32_t workgroups;
    int32_t zero_grad;
    int32_t n_groups;
    float lr[WJ_ADAMW_MAX_GROUPS];
    float weight_decay[WJ_ADAMW_MAX_GROUPS];
    const uint8_t* group_map;
    int64_t first;
} wj_adamw_groups_args;
int wj_adamw_groups_step(const wj_adamw_groups_args*, void* stream);

/* sizeof of a struct declared in this header by name (-1: unknown); scratch bytes of an entry declared here (0: the pass takes none;
 * -1: unknown entry) */
int wj_optim_struct_size(const char* name);
int64_t wj_optim_workspace_bytes(const char* fn, const void* args);

#ifdef __cplusplus
}
#endif
#endif /* WAVJEPA_HIP_OPTIM_H */
