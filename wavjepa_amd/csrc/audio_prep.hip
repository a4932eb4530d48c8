// Audio preparation on the device (reference data_modules/WebAudioDataModule.py:43-60 + dataset_functions.py:90-111):
//   raw integer PCM of a ragged batch -> float -> polyphase kaiser-sinc resampling (any rate pair) -> RMS -14 dBFS -> pad / cut.
//
// wj_audio_prepare is three passes per call, all on the caller's stream:
//   1. prep_fir_kernel / prep_copy_kernel: r = resample(x) written un-scaled into the output rows (o < out_len) and one partial
//      sum of squares per workgroup over ALL resampled samples (also those beyond out_len) into the workspace (plain stores);
//   2. prep_gain_kernel: one workgroup per clip adds that clip's partials in a fixed order (fp64) and stores the gain;
//   3. prep_scale_kernel: y = r * gain in place, zeros behind the clip.
// No float atomics: two launches give the same bits, and a clip's partial records depend on its own length and rate pair only.
//
// Pass 1 is a GEMM in disguise: out[frame i][phase p] = sum_k tab[p][k] * xpad[i * orig + k].  The tap table (815 x 160 floats at
// 44.1 -> 16 kHz) stays in global memory / L2; a workgroup takes (clip, FB frames, PT phases) and walks the taps in chunks of KC:
// per chunk it stages tab[PT][KC] and the input samples its frames need in LDS and every thread advances an FR x PR register tile
// (one LDS read feeds FR or PR FMAs: 4 x 4 for the many-phase pairs -- 8 ds_read_b32 per 16 FMAs, LDS-bound at a fifth of the fp32
// vector peak; an 8 x 8 tile halves the reads per FMA but measured HALF the rate: 138 VGPRs and a 42-KB workgroup leave three waves
// per SIMD and 384 workgroups per 32-clip batch, too few to hide the global loads of the staging -- and 4 x nw for pairs of up to
// four phases).  The window is staged CONTIGUOUSLY ((FB - 1) * orig + KC
// samples) when the frames overlap (orig small: 32 / 48 / 8 kHz) and GATHERED per frame ([FB][KC]) when they do not (orig = 441).
// LDS rows are padded to KC + 1
// floats: lanes that differ in the phase (table) or in the frame (gathered window) hit different banks of ds_read_b32.
// Every output is ONE fmaf chain over k ascending -- the order of wj_resample_fir, so the two agree bit for bit on the same input.
#include "stream_pieces.h"

namespace {

constexpr int KC = 32;            // taps per staged chunk
constexpr int KCP = KC + 1;       // padded LDS row
constexpr int CHUNK = 32;         // clips per launch (their descriptors travel as kernel arguments)
constexpr int COPY_BLOCK = 4096;  // samples per workgroup of the copy path
constexpr int MAX_PHASES = 1024, MAX_TAPS = 4096;
constexpr int WIDE_FB = 64;                           // wide tile: 16 x 16 threads, 4 frames x 4 phases each
constexpr int NARROW_FB = 1024, NARROW_WIN = 8192;    // narrow tiles: 256 threads, 4 frames x all (1 / 2 / 4) phases each, contiguous window only

struct prep_chunk {
    long off[CHUNK];     // first sample of the clip in the flat buffer
    int len[CHUNK];      // samples at the file rate
    float scale[CHUNK];  // 2^-(bits - 1), 1 for float input
    int index[CHUNK];    // output row
    int first;           // position of clip 0 of this chunk in the call's clip list (workspace row)
};

struct prep_dims {
    const void* pcm;
    const float* table;
    float* out;
    float* partials;     // [n_clips][parts_stride]
    float* gains;        // [n_clips]
    long parts_stride;
    int kind, orig, nw, width, taps, out_len, skip_normalize;
};

__device__ __forceinline__ float load_sample(const void* pcm, int kind, long i) {
    if (kind == 0) return (float)((const int16_t*)pcm)[i];
    if (kind == 1) return (float)((const int32_t*)pcm)[i];
    return ((const float*)pcm)[i];
}

__device__ __forceinline__ long resampled_len(int n, int orig, int nw) { return ((long)nw * n + orig - 1) / orig; }

// WIN: floats of the window buffer.  The gathered form needs FB * KCP of them; a tile without that room (the narrow ones) is only
// launched for rate pairs whose contiguous span fits (plan_for).
template <int TF, int TP, int FR, int PR, int WIN>
__global__ __launch_bounds__(TF * TP) void prep_fir_kernel(prep_dims d, prep_chunk c) {
    constexpr int FB = TF * FR, PT = TP * PR, NT = TF * TP;
    __shared__ float win[WIN];
    __shared__ float tab[PT * KCP];
    __shared__ float red[16];
    const int j = blockIdx.z;
    const int n = c.len[j];
    const long L_r = resampled_len(n, d.orig, d.nw);
    const long frames = (L_r + d.nw - 1) / d.nw;
    const long i0 = (long)blockIdx.x * FB;
    if (i0 >= frames) return;
    const int p0 = blockIdx.y * PT;
    const int tid = threadIdx.x, tp = tid % TP, tf = tid / TP;
    const long off = c.off[j];
    const float scale = c.scale[j];
    const bool contiguous = (long)(FB - 1) * d.orig + KC <= WIN;
    const int fstride = contiguous ? d.orig : KCP;
    float acc[FR][PR];
#pragma unroll
    for (int r = 0; r < FR; ++r)
#pragma unroll
        for (int q = 0; q < PR; ++q) acc[r][q] = 0.f;

    for (int k0 = 0; k0 < d.taps; k0 += KC) {
        const int kc = min(KC, d.taps - k0);
        for (int e = tid; e < PT * KC; e += NT) {
            const int pp = e / KC, kk = e % KC, p = p0 + pp;
            tab[pp * KCP + kk] = (p < d.nw && kk < kc) ? d.table[(long)p * d.taps + k0 + kk] : 0.f;
        }
        if (contiguous) {
            const int span = (FB - 1) * d.orig + KC;
            const long base = i0 * d.orig + k0 - d.width;
            for (int e = tid; e < span; e += NT) {
                const long src = base + e;
                win[e] = (src >= 0 && src < n) ? load_sample(d.pcm, d.kind, off + src) * scale : 0.f;
            }
        } else {
            for (int e = tid; e < FB * KC; e += NT) {
                const int f = e / KC, kk = e % KC;
                const long src = (i0 + f) * d.orig + k0 + kk - d.width;
                win[f * KCP + kk] = (src >= 0 && src < n) ? load_sample(d.pcm, d.kind, off + src) * scale : 0.f;
            }
        }
        __syncthreads();
        const float* wa = win + tf * fstride;
        const float* tb = tab + tp * KCP;
#pragma unroll 4
        for (int kk = 0; kk < kc; ++kk) {
            float av[FR], bv[PR];
#pragma unroll
            for (int r = 0; r < FR; ++r) av[r] = wa[r * TF * fstride + kk];
#pragma unroll
            for (int q = 0; q < PR; ++q) bv[q] = tb[q * TP * KCP + kk];
#pragma unroll
            for (int r = 0; r < FR; ++r)
#pragma unroll
                for (int q = 0; q < PR; ++q) acc[r][q] = fmaf(bv[q], av[r], acc[r][q]);
        }
        __syncthreads();
    }

    float* y = d.out + (long)c.index[j] * d.out_len;
    float ss = 0.f;
#pragma unroll
    for (int r = 0; r < FR; ++r)
#pragma unroll
        for (int q = 0; q < PR; ++q) {
            const int p = p0 + tp + q * TP;
            const long o = (i0 + tf + r * TF) * d.nw + p;
            if (p < d.nw && o < L_r) {
                const float v = acc[r][q];
                ss = fmaf(v, v, ss);
                if (o < d.out_len) y[o] = v;
            }
        }
    ss = block_sum(ss, red);
    if (tid == 0) d.partials[(long)(c.first + j) * d.parts_stride + (long)blockIdx.x * gridDim.y + blockIdx.y] = ss;
}

// orig == new: r = x.  One workgroup per COPY_BLOCK samples.
__global__ __launch_bounds__(256) void prep_copy_kernel(prep_dims d, prep_chunk c) {
    __shared__ float red[16];
    const int j = blockIdx.y;
    const int n = c.len[j];
    const long lo = (long)blockIdx.x * COPY_BLOCK;
    if (lo >= n) return;
    const long hi = min((long)n, lo + COPY_BLOCK);
    const long off = c.off[j];
    const float scale = c.scale[j];
    float* y = d.out + (long)c.index[j] * d.out_len;
    float ss = 0.f;
    for (long o = lo + threadIdx.x; o < hi; o += 256) {
        const float v = load_sample(d.pcm, d.kind, off + o) * scale;
        ss = fmaf(v, v, ss);
        if (o < d.out_len) y[o] = v;
    }
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) d.partials[(long)(c.first + j) * d.parts_stride + blockIdx.x] = ss;
}

// One workgroup per clip: the clip's partial records in a fixed order, fp64; gain = 10^((-14 - 20 log10 rms) / 20).
__global__ __launch_bounds__(256) void prep_gain_kernel(prep_dims d, prep_chunk c, int frame_block, int phase_tiles) {
    __shared__ double red[256];
    const int j = blockIdx.x;
    const long L_r = resampled_len(c.len[j], d.orig, d.nw);
    long parts;
    if (d.table) {
        const long frames = (L_r + d.nw - 1) / d.nw;
        parts = (frames + frame_block - 1) / frame_block * phase_tiles;
    } else {
        parts = (L_r + COPY_BLOCK - 1) / COPY_BLOCK;
    }
    const float* p = d.partials + (long)(c.first + j) * d.parts_stride;
    double s = 0.0;
    for (long i = threadIdx.x; i < parts; i += 256) s += (double)p[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float g = 1.f;
        if (!d.skip_normalize && L_r > 0 && red[0] > 0.0) {
            const double rms = sqrt(red[0] / (double)L_r);
            g = (float)pow(10.0, (-14.0 - 20.0 * log10(rms)) / 20.0);
        }
        d.gains[c.first + j] = g;
    }
}

__global__ __launch_bounds__(256) void prep_scale_kernel(prep_dims d, prep_chunk c) {
    const int j = blockIdx.y;
    const long L_r = resampled_len(c.len[j], d.orig, d.nw);
    const float g = d.gains[c.first + j];
    float* y = d.out + (long)c.index[j] * d.out_len;
    for_each_flat(d.out_len, [&](long o) { y[o] = o < L_r ? y[o] * g : 0.f; });
}

struct prep_plan {
    int variant;        // -1: copy path; 0..2: narrow tiles (1024 frames x 1 / 2 / 4 phases); 3: the wide tile (64 frames x 64 phases)
    int frame_block, phase_tiles;
    long parts_stride;  // partial records of the longest clip
};

bool plan_for(const wj_audio_prepare_args* a, prep_plan* pl) {
    const long L_r = ((long)a->nw * a->max_len + a->orig - 1) / a->orig;
    if (!a->table) {
        pl->variant = -1;
        pl->frame_block = COPY_BLOCK;
        pl->phase_tiles = 1;
        pl->parts_stride = (L_r + COPY_BLOCK - 1) / COPY_BLOCK;
    } else {
        int pt;
        const bool narrow = a->nw <= 4 && (long)(NARROW_FB - 1) * a->orig + KC <= NARROW_WIN;   // few phases, overlapping frames
        if (narrow && a->nw <= 1) pl->variant = 0, pt = 1, pl->frame_block = NARROW_FB;
        else if (narrow && a->nw <= 2) pl->variant = 1, pt = 2, pl->frame_block = NARROW_FB;
        else if (narrow) pl->variant = 2, pt = 4, pl->frame_block = NARROW_FB;
        else pl->variant = 3, pt = 64, pl->frame_block = WIDE_FB;
        pl->phase_tiles = (a->nw + pt - 1) / pt;
        const long frames = (L_r + a->nw - 1) / a->nw;
        pl->parts_stride = (frames + pl->frame_block - 1) / pl->frame_block * pl->phase_tiles;
    }
    if (pl->parts_stride < 1) pl->parts_stride = 1;
    return true;
}

// argument errors that need no device
int check_dims(const wj_audio_prepare_args* a) {
    if (a->B <= 0 || a->n_clips <= 0 || a->out_len <= 0 || a->max_len < 0 || a->orig <= 0 || a->nw <= 0) return WJ_ERR_ARG;
    if (a->pcm_kind < 0 || a->pcm_kind > 2) return WJ_ERR_ARG;
    if (a->table) {
        if (a->width < 0 || a->taps != 2 * a->width + a->orig) return WJ_ERR_ARG;
        if (a->nw > MAX_PHASES || a->taps > MAX_TAPS) return WJ_ERR_UNSUPPORTED;
    } else if (a->orig != a->nw) {
        return WJ_ERR_ARG;
    }
    return WJ_OK;
}

}  // namespace

int64_t wj_audio_prepare_ws_bytes(const wj_audio_prepare_args* a) {
    if (check_dims(a) != WJ_OK) return -1;
    prep_plan pl;
    plan_for(a, &pl);
    return ((int64_t)a->n_clips * pl.parts_stride + a->n_clips) * 4;
}

extern "C" int wj_audio_prepare(const wj_audio_prepare_args* a, void* stream) {
    const CheckedEntry entry(__func__);
    if (!a || !a->pcm || !a->offsets || !a->lengths || !a->clips || !a->out || !a->workspace) return WJ_ERR_ARG;
    if (a->pcm_kind != 2 && !a->bits) return WJ_ERR_ARG;
    const int rc = check_dims(a);
    if (rc != WJ_OK) return rc;
    for (int j = 0; j < a->n_clips; ++j) {
        const int b = a->clips[j];
        if (b < 0 || b >= a->B) return WJ_ERR_ARG;
        if (a->lengths[b] < 0 || a->lengths[b] > a->max_len) return WJ_ERR_ARG;
        if (a->offsets[b] < 0 || a->offsets[b] + a->lengths[b] > a->pcm_elems) return WJ_ERR_ARG;
        if (a->pcm_kind != 2 && (a->bits[b] < 8 || a->bits[b] > 32 || (a->pcm_kind == 0 && a->bits[b] > 16))) return WJ_ERR_ARG;
    }
    prep_plan pl;
    plan_for(a, &pl);
    if (a->workspace_bytes < ((int64_t)a->n_clips * pl.parts_stride + a->n_clips) * 4) return WJ_ERR_ARG;

    hipStream_t st = (hipStream_t)stream;
    prep_dims d;
    d.pcm = a->pcm;
    d.table = a->table;
    d.out = a->out;
    d.partials = (float*)a->workspace;
    d.gains = d.partials + (long)a->n_clips * pl.parts_stride;
    d.parts_stride = pl.parts_stride;
    d.kind = a->pcm_kind;
    d.orig = a->orig;
    d.nw = a->nw;
    d.width = a->width;
    d.taps = a->taps;
    d.out_len = a->out_len;
    d.skip_normalize = a->skip_normalize;
    for (int first = 0; first < a->n_clips; first += CHUNK) {
        const int m = a->n_clips - first < CHUNK ? a->n_clips - first : CHUNK;
        prep_chunk c;
        int longest = 0;
        for (int j = 0; j < CHUNK; ++j) {
            const int b = a->clips[first + (j < m ? j : 0)];
            c.off[j] = a->offsets[b];
            c.len[j] = a->lengths[b];
            c.scale[j] = a->pcm_kind == 2 ? 1.0f : 1.0f / (float)(1LL << (a->bits[b] - 1));
            c.index[j] = b;
            if (j < m && c.len[j] > longest) longest = c.len[j];
        }
        c.first = first;
        const long L_r = ((long)a->nw * longest + a->orig - 1) / a->orig;
        if (L_r > 0) {
            if (pl.variant < 0) {
                hipLaunchKernelGGL(prep_copy_kernel, dim3((unsigned)((L_r + COPY_BLOCK - 1) / COPY_BLOCK), m), dim3(256), 0, st, d, c);
            } else {
                const long frames = (L_r + a->nw - 1) / a->nw;
                const dim3 grid((unsigned)((frames + pl.frame_block - 1) / pl.frame_block), pl.phase_tiles, m);
                if (pl.variant == 0) hipLaunchKernelGGL((prep_fir_kernel<256, 1, 4, 1, NARROW_WIN>), grid, dim3(256), 0, st, d, c);
                else if (pl.variant == 1) hipLaunchKernelGGL((prep_fir_kernel<256, 1, 4, 2, NARROW_WIN>), grid, dim3(256), 0, st, d, c);
                else if (pl.variant == 2) hipLaunchKernelGGL((prep_fir_kernel<256, 1, 4, 4, NARROW_WIN>), grid, dim3(256), 0, st, d, c);
                else hipLaunchKernelGGL((prep_fir_kernel<16, 16, 4, 4, WIDE_FB * KCP>), grid, dim3(256), 0, st, d, c);
            }
        }
        hipLaunchKernelGGL(prep_gain_kernel, dim3(m), dim3(256), 0, st, d, c, pl.frame_block, pl.phase_tiles);
        hipLaunchKernelGGL(prep_scale_kernel, dim3((unsigned)((a->out_len + 1023) / 1024), m), dim3(256), 0, st, d, c);
    }
    return entry.launched();
}
