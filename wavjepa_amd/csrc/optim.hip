// libwavjepa_hip_optim.so (include/wavjepa_hip_optim.h): wj_adamw_groups_step, the AdamW pass with a learning rate and a weight decay
// per parameter group, and the library's two query entries.
//
// The pass is adamw_kernel's (csrc/misc.hip): one f32x4 of p, g, m, v per thread and iteration, 16-byte accesses, the grid-stride loop
// of 256-thread workgroups, the `workgroups` cap, the fused clear of g and the bf16 shadow; the element update is the one copy in
// csrc/stream_pieces.h (adamw_clip_coef / adamw_rates / adamw_update4), so an element of group k has the bits wj_adamw_step gives it
// with that group's pair.  What is new is the lookup:
//   * the group of an element comes from one byte per 8-element granule of the flat layout (n / 8 bytes beside 28 .. 34 n bytes of
//     stream: under 0.5 %).  Thread i (one f32x4) reads byte i / 2: a wave reads 32 consecutive bytes, one request, issued with the
//     four 16-byte loads of the iteration and independent of them;
//   * the byte indexes a table of (decay, step) in LDS that every workgroup forms once from the by-value lr[] / weight_decay[] of its
//     arguments (64 threads, one division each).  No search, no second global load behind the byte: the dependent read is an LDS read
//     of 8 bytes, two lanes per address, while the iteration's global loads are in flight;
//   * a workgroup issues its first iteration's loads BEFORE it forms the table: formed in front of them the table cost 9 us of 634 at
//     the full grid (8192 workgroups of ~13 iterations), formed under their latency the pass takes the parent's time
//     (profiles/param_groups.txt: 628.4 us against 628.4 us at the full grid, 602.8 against 603.6 at 256 workgroups).
#include "stream_pieces.h"
#include "../../include/wavjepa_hip_optim.h"
#include "abi_queries.h"

namespace {

// the loads of one iteration (and, with zero_grad, the clear behind the read of g): thread i's f32x4 of p, g, m, v and its granule's group
__device__ __forceinline__ void adamw_groups_fetch(const wj_adamw_groups_args& a, const uint8_t* map, long i, int& k, f32x4& p, f32x4& g,
                                                   f32x4& m, f32x4& v) {
    k = map[i >> 1] & (WJ_ADAMW_MAX_GROUPS - 1);
    p = *reinterpret_cast<const f32x4*>(a.p + i * 4);
    g = *reinterpret_cast<const f32x4*>(a.g + i * 4);
    if (a.zero_grad) *reinterpret_cast<f32x4*>(a.g + i * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    m = *reinterpret_cast<const f32x4*>(a.m + i * 4);
    v = *reinterpret_cast<const f32x4*>(a.v + i * 4);
}

__global__ __launch_bounds__(256) void adamw_groups_kernel(wj_adamw_groups_args a) {
    __shared__ float2 rates[WJ_ADAMW_MAX_GROUPS];          // (decay, step) per group
    const long n4 = a.n / 4;
    const long stride = (long)gridDim.x * 256;
    const uint8_t* map = a.group_map + a.first / WJ_ADAMW_GRANULE;
    long i = blockIdx.x * 256L + threadIdx.x;
    int k = 0;
    f32x4 p, g, m, v;
    // the first iteration's loads are issued in front of the table: a workgroup's prologue (64 loads of its arguments, a division, a
    // barrier) then runs under their latency instead of in front of it -- at the full grid a workgroup has only ~13 iterations to hide it in
    if (i < n4) adamw_groups_fetch(a, map, i, k, p, g, m, v);
    if (threadIdx.x < WJ_ADAMW_MAX_GROUPS) {
        const int q = threadIdx.x < a.n_groups ? threadIdx.x : 0;      // (rows past n_groups repeat group 0: never read by a valid map)
        float decay, step;
        adamw_rates(a.lr[q], a.weight_decay[q], a.bc1, decay, step);
        rates[threadIdx.x] = float2{decay, step};
    }
    const float coef = adamw_clip_coef(a.sumsq, a.max_norm, a.grad_scale);
    const float rbc2 = rsqrtf(a.bc2);
    __syncthreads();
    while (i < n4) {
        const float2 r = rates[k];
        adamw_update4(p, g, m, v, coef, r.x, r.y, rbc2, a.beta1, a.beta2, a.eps);
        *reinterpret_cast<f32x4*>(a.p + i * 4) = p;
        *reinterpret_cast<f32x4*>(a.m + i * 4) = m;
        *reinterpret_cast<f32x4*>(a.v + i * 4) = v;
        if (a.p_bf16) *reinterpret_cast<bf16x4*>((bf16_t*)a.p_bf16 + i * 4) = to_bf16x4(p);
        i += stride;
        if (i < n4) adamw_groups_fetch(a, map, i, k, p, g, m, v);
    }
}

}  // namespace

extern "C" WJ_EXPORT int wj_adamw_groups_step(const wj_adamw_groups_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->p || !a->g || !a->m || !a->v || !a->group_map) return WJ_ERR_ARG;
    if (a->n <= 0 || (a->n & (WJ_ADAMW_GRANULE - 1)) || a->first < 0 || (a->first & (WJ_ADAMW_GRANULE - 1))) return WJ_ERR_ARG;
    if (a->n_groups < 1 || a->n_groups > WJ_ADAMW_MAX_GROUPS) return WJ_ERR_ARG;
    if ((((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v) & 15) || ((uintptr_t)a->p_bf16 & 7)) return WJ_ERR_ARG;
    int grid = grid_for(a->n / 4, 256);
    if (a->workgroups > 0 && a->workgroups < grid) grid = a->workgroups;
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *a);
    return entry.launched();
}

WJ_ABI_QUERIES(WJ_OPTIM_ENTRIES, WJ_OPTIM_OTHER_STRUCTS, wj_optim_struct_size, wj_optim_workspace_bytes)
