// libwavjepa_hip_monitor.so (include/wavjepa_hip_monitor.h): wj_masked_moments, the collapse monitor behind the masked loss, and the
// library's two query entries, generated from its rows of the entry table (csrc/abi_table.h) as csrc/abi.hip generates libwavjepa_hip.so's.
//
// HBM-bound: the pass reads what the loss reads (the target rows of preds and targets) and writes about 1 MB of records.
//   pass 1  grid (row groups of MROWS, column slabs of MCOLS), 256 threads = 32 row slots x 8 chunks of 8 columns (one 16-byte load of
//           bf16 preds, two of fp32 targets).  The group's row list and mask bytes are staged once in LDS (y_row), so the row loop waits
//           for its data loads only.  Thread (slot, chunk) takes rows slot, slot + 32, ... of its group, MFLIGHT in flight.  All
//           sums are fp64 and shifted by the first target value the thread saw: s1 = sum (x - k), s2 = sum (x - k)^2, so that
//           M2 = s2 - s1^2 / n loses nothing to a mean far above the spread and is exactly 0 for a constant column.  The 32 slots are
//           merged in LDS (Chan, slots 0..15, slots 16..31, then the two halves) into one record per workgroup.
//   pass 2  one workgroup of 1024: the Chan factors of the row-group counts once (they are the same for every column), then one chain
//           over the row groups in ascending order per (tensor, column), the two scalars through a fixed pairwise tree, and col.
// fp64 throughout because the bound the tests hold this to is about one fp32 ulp of the variance (PARITY.md): fp32 partials of 32
// rows do not stay inside it, and at 5 fp64 instructions per element the pass is nowhere near the fp64 rate.  Measured
// (profiles/monitor.txt): pass 1 47 us at the step's shape, pass 2 33 us -- one CU reading the records from the Infinity Cache.
#include "stream_pieces.h"
#include "../../include/wavjepa_hip_monitor.h"
#include "abi_queries.h"

namespace {

constexpr int MROWS = WJ_MOMENTS_ROWS, MCOLS = WJ_MOMENTS_COLS, MCHUNKS = MCOLS / 8, MSLOTS = 256 / MCHUNKS, MAXG = WJ_MOMENTS_MAX_GROUPS;
constexpr int MFLIGHT = 4;         // rows a thread has in flight
constexpr int MPAD = 256 + 8;       // LDS row of the slot merge: 8 values x 8 chunks of one slot land in 64 different doubles
static_assert(MROWS % (MFLIGHT * MSLOTS) == 0 && MCHUNKS == 8 && MSLOTS == 32, "thread layout of moments_rows_kernel");

// Chan's merge of (n, m, M2) with (nb, mb, M2b): f1 = nb / (n + nb), f2 = n nb / (n + nb).  An empty side needs no case of its own:
// its mean and M2 are 0, with n = 0 the factors are (1, 0) and m = 0 + mb exactly.  Equal means leave m and add M2b only.
__device__ __forceinline__ void chan_factors(double n, double nb, double& f1, double& f2) {
    const double nt = n + nb;
    f1 = nt > 0.0 ? nb / nt : 0.0;
    f2 = nt > 0.0 ? n * nb / nt : 0.0;
}
__device__ __forceinline__ void chan_merge(double& m, double& M2, double mb, double M2b, double f1, double f2) {
    const double d = mb - m;
    m += d * f1;
    M2 += M2b + d * d * f2;
}

// eight columns of one thread: shift k (an input value, so exact in fp32), s1 = sum (x - k), s2 = sum (x - k)^2
struct Shifted8 {
    float k[8];
    double s1[8], s2[8];
};
__device__ __forceinline__ void shifted_add(Shifted8& a, f32x4 lo, f32x4 hi, bool first) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = e < 4 ? lo[e] : hi[e - 4];
        a.k[e] = first ? x : a.k[e];
        const double d = (double)x - (double)a.k[e];
        a.s1[e] += d;
        a.s2[e] = fma(d, d, a.s2[e]);
    }
}

__global__ __launch_bounds__(256, 3) void moments_rows_kernel(wj_moments_args a, long R, int gx, int Dp) {
    __shared__ double sh[16][MPAD];
    __shared__ double half_m[2][MCOLS], half_M2[2][MCOLS];
    __shared__ double slot_f1[MSLOTS], slot_f2[MSLOTS], half_f[2], group_n;
    __shared__ int y_row[MROWS];                        // row b*T + t of targets for every row of the group; -1: not a target (or past R)
    __shared__ int slot_n[MSLOTS];
    const int tid = threadIdx.x, chunk = tid & (MCHUNKS - 1), slot = tid >> 3;
    const int D = a.D, col0 = blockIdx.y * MCOLS + chunk * 8;
    const bool active = col0 < D;                       // (chunk 0 of every slab is: the grid has ceil(D / MCOLS) slabs)
    const long base = (long)blockIdx.x * MROWS;
    // the group's row list and mask once, coalesced: the loop below then waits for its data loads only
    for (int j = tid; j < MROWS; j += 256) {
        const long r = base + j;
        int v = -1;
        if (r < R) {
            const uint32_t dense = a.rows ? (uint32_t)a.rows[r] : (uint32_t)r;       // (b*G+g)*T + t; preds are indexed by r
            if (a.tgt[dense] != 0) {
                const uint32_t bg = dense / (uint32_t)a.T;
                v = (int)((bg / (uint32_t)a.G) * (uint32_t)a.T + (dense - bg * (uint32_t)a.T));
            }
        }
        y_row[j] = v;
    }
    __syncthreads();
    Shifted8 p, y;
#pragma unroll
    for (int e = 0; e < 8; ++e) p.k[e] = y.k[e] = 0.f, p.s1[e] = p.s2[e] = y.s1[e] = y.s2[e] = 0.0;
    int cnt = 0;
    const bf16_t* pbase = (const bf16_t*)a.preds + base * D + col0;
    const float* ybase = a.targets + col0;
    for (int j0 = slot; j0 < MROWS && base + j0 < R; j0 += MFLIGHT * MSLOTS) {
        int yr[MFLIGHT];
#pragma unroll
        for (int u = 0; u < MFLIGHT; ++u) yr[u] = active ? y_row[j0 + u * MSLOTS] : -1;
        bf16x8 pv[MFLIGHT];
        f32x4 y0[MFLIGHT], y1[MFLIGHT];
#pragma unroll
        for (int u = 0; u < MFLIGHT; ++u)
            if (yr[u] >= 0) {
                pv[u] = *reinterpret_cast<const bf16x8*>(pbase + (long)(j0 + u * MSLOTS) * D);
                y0[u] = *reinterpret_cast<const f32x4*>(ybase + (long)yr[u] * D);
                y1[u] = *reinterpret_cast<const f32x4*>(ybase + (long)yr[u] * D + 4);
            }
#pragma unroll
        for (int u = 0; u < MFLIGHT; ++u)
            if (yr[u] >= 0) {
                const bf16x4 lo = {pv[u][0], pv[u][1], pv[u][2], pv[u][3]}, hi = {pv[u][4], pv[u][5], pv[u][6], pv[u][7]};
                shifted_add(p, to_f32x4(lo), to_f32x4(hi), cnt == 0);
                shifted_add(y, y0[u], y1[u], cnt == 0);
                ++cnt;
            }
    }
    if (chunk == 0) slot_n[slot] = cnt;
    const double inv = cnt ? 1.0 / (double)cnt : 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const Shifted8& s = q ? y : p;
        __syncthreads();                                 // slot_n written (q = 0); sh and half_* read (q = 1)
        if (q == 0 && tid < MSLOTS) {                    // the factors of the slot merge, the same for every column
            double before = 0.0;
            for (int sl = tid & 16; sl < tid; ++sl) before += (double)slot_n[sl];
            chan_factors(before, (double)slot_n[tid], slot_f1[tid], slot_f2[tid]);
            if (tid == 0) {
                double n0 = 0.0, n1 = 0.0;
                for (int sl = 0; sl < 16; ++sl) n0 += (double)slot_n[sl], n1 += (double)slot_n[16 + sl];
                chan_factors(n0, n1, half_f[0], half_f[1]);
                group_n = n0 + n1;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sh[e][tid] = cnt ? (double)s.k[e] + s.s1[e] * inv : 0.0;
            sh[8 + e][tid] = cnt ? fmax(s.s2[e] - s.s1[e] * s.s1[e] * inv, 0.0) : 0.0;
        }
        __syncthreads();
        const int e = (tid >> 3) & 7, ch = tid & 7, half = tid >> 6;       // tid < 128: column ch * 8 + e of the slab, slots half * 16 ..
        double m = 0.0, M2 = 0.0;
        if (tid < 128) {
            for (int s16 = 0; s16 < 16; ++s16) {
                const int sl = half * 16 + s16;
                chan_merge(m, M2, sh[e][sl * 8 + ch], sh[8 + e][sl * 8 + ch], slot_f1[sl], slot_f2[sl]);
            }
            half_m[half][ch * 8 + e] = m;
            half_M2[half][ch * 8 + e] = M2;
        }
        __syncthreads();
        if (tid < 64) {
            chan_merge(m, M2, half_m[1][ch * 8 + e], half_M2[1][ch * 8 + e], half_f[0], half_f[1]);
            const int c = blockIdx.y * MCOLS + ch * 8 + e;
            if (c < D) {
                double* rec = a.workspace + gx + ((long)blockIdx.x * 2 + q) * 2 * Dp + c;
                rec[0] = m;
                rec[Dp] = M2;
            }
            if (q == 0 && tid == 0 && blockIdx.y == 0) a.workspace[blockIdx.x] = group_n;
        }
    }
}

__global__ __launch_bounds__(1024) void moments_final_kernel(wj_moments_args a, int gx, int Dp) {
    __shared__ double cn[MAXG], f1[MAXG], f2[MAXG];
    const int tid = threadIdx.x, D = a.D;
    for (int i = tid; i < gx; i += 1024) cn[i] = a.workspace[i];
    __syncthreads();
    for (int i = tid; i < gx; i += 1024) {
        double before = 0.0;                             // (counts are integers: exact in any order)
        for (int j = 0; j < i; ++j) before += cn[j];
        chan_factors(before, cn[i], f1[i], f2[i]);
    }
    __syncthreads();
    double n = 0.0;
    for (int i = 0; i < gx; ++i) n += cn[i];
    double acc[2] = {0.0, 0.0};
    for (int pc = tid; pc < 2 * D; pc += 1024) {
        const int q = pc >= D ? 1 : 0, c = pc - q * D;
        const double* rec = a.workspace + gx + (long)q * 2 * Dp + c;
        double m = 0.0, M2 = 0.0;
#pragma unroll 16
        for (int i = 0; i < gx; ++i) chan_merge(m, M2, rec[(long)i * 4 * Dp], rec[(long)i * 4 * Dp + Dp], f1[i], f2[i]);
        if (a.col) {
            a.col[((long)q * 2) * D + c] = m;
            a.col[((long)q * 2 + 1) * D + c] = M2;
        }
        acc[q] += sqrt((n >= 2.0 ? M2 / (n - 1.0) : 0.0) + 1e-6);
    }
    __syncthreads();                                     // the factors are read no more: their arrays hold the tree
    f1[tid] = acc[0];
    f2[tid] = acc[1];
    for (int s = 512; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            f1[tid] += f1[tid + s];
            f2[tid] += f2[tid + s];
        }
    }
    if (tid == 0) {
        a.out[0] = (float)(f1[0] / (double)D);
        a.out[1] = (float)(f2[0] / (double)D);
        a.out[2] = (float)n;
        a.out[3] = 0.f;
    }
}

inline long moments_groups(long R) { return (R + MROWS - 1) / MROWS; }
inline int moments_padded(int D) { return (D + MCOLS - 1) / MCOLS * MCOLS; }

}  // namespace

// count per row group, then per row group [2 tensors][mean | M2][D padded to the slab]; sized for the longest row list of the shape
int64_t wj_masked_moments_ws_bytes(const wj_moments_args* a) {
    if (a->B < 0 || a->G < 0 || a->T < 0 || a->D < 0 || a->n_rows < 0) return -1;
    const long dense = (long)a->B * a->G * a->T;
    const long gx = moments_groups(dense > a->n_rows ? dense : (long)a->n_rows);
    return 8 * (gx + 4 * gx * (int64_t)moments_padded(a->D));
}

extern "C" WJ_EXPORT int wj_masked_moments(const wj_moments_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->preds || !a->targets || !a->tgt || !a->out || !a->workspace) return WJ_ERR_ARG;
    if (a->B <= 0 || a->G <= 0 || a->T <= 0 || a->D <= 0 || (a->rows && a->n_rows < 0)) return WJ_ERR_ARG;
    if (((uintptr_t)a->preds & 15) || ((uintptr_t)a->targets & 15) || ((uintptr_t)a->workspace & 7) || ((uintptr_t)a->col & 7) ||
        ((uintptr_t)a->out & 3) || ((uintptr_t)a->rows & 3))
        return WJ_ERR_ARG;
    if (a->D & 7) return WJ_ERR_UNSUPPORTED;
    const long R = a->rows ? (long)a->n_rows : (long)a->B * a->G * a->T;
    const long gx = moments_groups(R);
    if (gx > MAXG) return WJ_ERR_UNSUPPORTED;
    const int Dp = moments_padded(a->D);
    if (gx > 0) hipLaunchKernelGGL(moments_rows_kernel, dim3((unsigned)gx, Dp / MCOLS), dim3(256), 0, (hipStream_t)stream, *a, R, (int)gx, Dp);
    hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *a, (int)gx, Dp);
    return entry.launched();
}

WJ_ABI_QUERIES(WJ_MONITOR_ENTRIES, WJ_MONITOR_OTHER_STRUCTS, wj_monitor_struct_size, wj_monitor_workspace_bytes)
