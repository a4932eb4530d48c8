// Noise-clip preparation of the denoiser stage on the device (reference data_modules/dataset_functions.py pre_process_noise,
// scene_module/generate_scenes.py:132-154 the cut / fades, WebAudioDataModuleDenoiser.py:228-243 the placement):
//   ragged batch of f32 noise clips at the target rate -> RMS -14 dBFS over the WHOLE clip -> cut (longer than the row) or
//   fade-in + placement (shorter) -> fade-out -> rows of the [B][out_len] tensor scene.generate_scene takes as `noise`.
//
// wj_noise_prepare is two passes per call, both on the caller's stream, both HBM-bound:
//   1. noise_sumsq_kernel: one workgroup per SUM_BLOCK samples of a clip; every thread walks groups of four consecutive samples
//      (clip-relative, so the grouping does not depend on where the clip sits in the flat buffer), one fmaf chain per thread,
//      wave64 shuffles + LDS across the workgroup, one partial per workgroup into the workspace (plain store);
//   2. noise_write_kernel: every workgroup adds its clip's partials in a fixed order (fp64), forms the gain, and writes ROW_BLOCK
//      outputs of the row: zeros in front of and behind the clip, g * x in the interior, the ramps at the ends.  The whole row is
//      written, so no memset is needed.
// No float atomics; a clip's partial records depend on its own samples only: two launches give the same bits and a row does not
// depend on the other clips of the batch.
// Loads and stores are 16 bytes per lane (global_load / global_store_dwordx4).  The vector type below is declared 4-byte aligned:
// a clip starts anywhere in the flat buffer and is placed anywhere in its row, so source and destination are rarely both
// 16-byte aligned; the memory pipeline takes dword-aligned dwordx4 accesses, and where the ragged offset allows (the loader
// rounds every clip's offset up to four floats) they are aligned.  The last 1..3 samples of a block and every group that touches
// a row edge or a ramp go element by element.
#include "stream_pieces.h"

namespace {

constexpr int CHUNK = 64;          // clips per launch (their descriptors travel as kernel arguments)
constexpr int SUM_BLOCK = 16384;   // samples per workgroup of pass 1: 256 threads x 16 groups of 4
constexpr int ROW_BLOCK = 8192;    // outputs per workgroup of pass 2: 256 threads x 8 groups of 4

typedef float vec4u __attribute__((ext_vector_type(4), aligned(4)));

struct noise_chunk {
    long off[CHUNK];     // first sample of the clip in the flat buffer
    int len[CHUNK];      // n
    int cut[CHUNK];      // s (n > out_len), else 0
    int place[CHUNK];    // p (n <= out_len), else 0
    int index[CHUNK];    // output row
    int first;           // position of clip 0 of this chunk in the call's clip list (workspace row)
};

struct noise_dims {
    const float* noise;
    float* out;
    float* partials;     // [n_clips][parts_stride]
    long parts_stride;
    int out_len, fade_len;
};

__global__ __launch_bounds__(256) void noise_sumsq_kernel(noise_dims d, noise_chunk c) {
    __shared__ float red[16];
    const int j = blockIdx.y;
    const int n = c.len[j];
    const long lo = (long)blockIdx.x * SUM_BLOCK;
    if (lo >= n) return;
    const int cnt = (int)min((long)SUM_BLOCK, (long)n - lo);
    const float* x = d.noise + c.off[j] + lo;
    float ss = 0.f;
    int e = (int)threadIdx.x * 4;
#pragma unroll 4
    for (; e + 4 <= cnt; e += 1024) {
        const vec4u v = *(const vec4u*)(x + e);
        ss = fmaf(v.x, v.x, ss);
        ss = fmaf(v.y, v.y, ss);
        ss = fmaf(v.z, v.z, ss);
        ss = fmaf(v.w, v.w, ss);
    }
    for (; e < cnt; ++e) ss = fmaf(x[e], x[e], ss);      // the 1..3 samples behind the last whole group (one thread)
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) d.partials[(long)(c.first + j) * d.parts_stride + blockIdx.x] = ss;
}

// one output sample: i = position inside the placed clip (0 <= i < m), xs = the clip from its cut position on
__device__ __forceinline__ float noise_sample(const float* xs, int i, int m, int F, bool cut, float g) {
    float v = g * xs[i];
    const float den = (float)(F - 1);
    if (!cut && i < F) v *= F > 1 ? (float)i / den : 0.f;                       // torch.linspace(0, 1, F)
    if (i >= m - F) v *= F > 1 ? (float)(F - 1 - (i - (m - F))) / den : 1.f;    // torch.linspace(1, 0, F)
    return v;
}

__global__ __launch_bounds__(256) void noise_write_kernel(noise_dims d, noise_chunk c) {
    __shared__ double red[256];
    __shared__ float gain;
    const int j = blockIdx.y;
    const int n = c.len[j], T = d.out_len, F = d.fade_len;
    // the clip's partials in a fixed order, fp64 (every workgroup of the row forms the same gain)
    const long parts = ((long)n + SUM_BLOCK - 1) / SUM_BLOCK;
    const float* pp = d.partials + (long)(c.first + j) * d.parts_stride;
    double s = 0.0;
    for (long i = threadIdx.x; i < parts; i += 256) s += (double)pp[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // 10^((-14 - 20 log10 rms) / 20) = 10^(-14 / 20) / rms
        gain = red[0] > 0.0 ? (float)(0.19952623149688797 / sqrt(red[0] / (double)n)) : 1.f;
    }
    __syncthreads();
    const float g = gain;

    const bool cut = n > T;
    const int m = cut ? T : n;
    const int p = cut ? 0 : c.place[j];
    const float* xs = d.noise + c.off[j] + (cut ? c.cut[j] : 0);
    float* y = d.out + (long)c.index[j] * T;
    const int plain_lo = cut ? 0 : F, plain_hi = m - F;      // i in [plain_lo, plain_hi): no ramp
    const long base = (long)blockIdx.x * ROW_BLOCK;
#pragma unroll 2
    for (int e = (int)threadIdx.x * 4; e < ROW_BLOCK; e += 1024) {
        const long o = base + e;
        if (o >= T) break;
        const long i = o - p;
        if (o + 4 <= T && (i + 4 <= 0 || i >= m)) {
            *(vec4u*)(y + o) = vec4u{0.f, 0.f, 0.f, 0.f};
        } else if (o + 4 <= T && i >= plain_lo && i + 4 <= plain_hi) {
            const vec4u v = *(const vec4u*)(xs + i);
            *(vec4u*)(y + o) = vec4u{g * v.x, g * v.y, g * v.z, g * v.w};
        } else {
            for (int k = 0; k < 4 && o + k < T; ++k) {
                const long ik = i + k;
                y[o + k] = (ik >= 0 && ik < m) ? noise_sample(xs, (int)ik, m, F, cut, g) : 0.f;
            }
        }
    }
}

// argument errors that need no device
int check_dims(const wj_noise_prepare_args* a) {
    if (a->B <= 0 || a->n_clips <= 0 || a->out_len <= 0 || a->fade_len <= 0 || a->max_len <= 0) return WJ_ERR_ARG;
    if (a->out_len < a->fade_len || a->max_len < a->fade_len) return WJ_ERR_ARG;
    return WJ_OK;
}

long parts_stride_for(const wj_noise_prepare_args* a) { return ((long)a->max_len + SUM_BLOCK - 1) / SUM_BLOCK; }

}  // namespace

int64_t wj_noise_prepare_ws_bytes(const wj_noise_prepare_args* a) {
    if (check_dims(a) != WJ_OK) return -1;
    return (int64_t)a->n_clips * parts_stride_for(a) * 4;
}

extern "C" int wj_noise_prepare(const wj_noise_prepare_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->noise || !a->out || !a->workspace || !a->offsets || !a->lengths || !a->cut_start || !a->place_start || !a->clips)
        return WJ_ERR_ARG;
    const int rc = check_dims(a);
    if (rc != WJ_OK) return rc;
    const int T = a->out_len, F = a->fade_len;
    for (int j = 0; j < a->n_clips; ++j) {
        const int b = a->clips[j];
        if (b < 0 || b >= a->B) return WJ_ERR_ARG;
        const int n = a->lengths[b];
        if (n < F || n > a->max_len) return WJ_ERR_ARG;
        if (a->offsets[b] < 0 || a->offsets[b] + n > a->noise_elems) return WJ_ERR_ARG;
        if (n > T) {
            if (a->cut_start[b] < 0 || a->cut_start[b] >= n - T) return WJ_ERR_ARG;
        } else if (a->place_start[b] < 0 || a->place_start[b] > T - n) {
            return WJ_ERR_ARG;
        }
    }
    const long stride = parts_stride_for(a);
    if (a->workspace_bytes < (int64_t)a->n_clips * stride * 4) return WJ_ERR_ARG;

    hipStream_t st = (hipStream_t)stream;
    noise_dims d;
    d.noise = a->noise;
    d.out = a->out;
    d.partials = (float*)a->workspace;
    d.parts_stride = stride;
    d.out_len = T;
    d.fade_len = F;
    for (int first = 0; first < a->n_clips; first += CHUNK) {
        const int m = a->n_clips - first < CHUNK ? a->n_clips - first : CHUNK;
        noise_chunk c;
        int longest = 0;
        for (int j = 0; j < CHUNK; ++j) {
            const int b = a->clips[first + (j < m ? j : 0)];
            const int n = a->lengths[b];
            c.off[j] = a->offsets[b];
            c.len[j] = n;
            c.cut[j] = n > T ? a->cut_start[b] : 0;
            c.place[j] = n > T ? 0 : a->place_start[b];
            c.index[j] = b;
            if (j < m && n > longest) longest = n;
        }
        c.first = first;
        hipLaunchKernelGGL(noise_sumsq_kernel, dim3((unsigned)(((long)longest + SUM_BLOCK - 1) / SUM_BLOCK), m), dim3(256), 0, st, d, c);
        hipLaunchKernelGGL(noise_write_kernel, dim3((unsigned)(((long)T + ROW_BLOCK - 1) / ROW_BLOCK), m), dim3(256), 0, st, d, c);
    }
    return entry.launched();
}
