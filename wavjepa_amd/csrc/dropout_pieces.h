// The dropout mask generator, one definition for every site (csrc/dropout.hip, csrc/norm.hip, csrc/attention_stream.hip).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants
// 0x9E3779B9 / 0xBB67AE85.  Stateless: a mask is a pure function of (seed, call, stream_id, element), so the backward and the second
// forward of recompute mode regenerate it and nothing about it is ever stored.
//   key     = the 64-bit seed (the host mixes the data-parallel rank in): (low word, high word)
//   counter = (group low, group high, stream_id = site | layer << 8 | stack << 16, call)
// One call yields 128 bits = EIGHT 16-bit draws: draw j is bits [16 (j & 1), 16 (j & 1) + 16) of output word j >> 1.  An element is
// kept iff its draw >= thr, thr = round(p * 65536) (at most 65535); the rate that is drawn is thr / 65536 and the survivors are scaled
// by 65536 / (65536 - thr) in fp32 -- the scale of the rate that is actually drawn, so quantising p leaves no bias.
//
// Groups of eight.
//   row-major sites (residual adds, FFN): element (row, col) of the [M][N] tensor the launch addresses, N % 8 == 0:
//       group = row * (N / 8) + col / 8, draw = col % 8.
//   attention: element (sequence b of the launch, head h, query q, key k), H heads:
//       group = (((b * H + h) * 1024 + q) * 128) + (k / 32) * 4 + (k % 16) / 4,   draw = 4 * ((k % 32) / 16) + k % 4
//     i.e. the keys 32 c + 4 g + {0..3} and 32 c + 16 + 4 g + {0..3} of one query share a call: the eight probabilities that lane group
//     g of a wave holds for one query in the bf16 B operand of the P.V MFMA (two 16-key score tiles packed by pack_tiles).  The strides
//     1024 (queries) and 128 (key groups) are the family's longest sequence, not the launch's T, so the mask of (b, h, q, k) does not
//     depend on T, on the 128-key blocking or on which kernel phase asks for it.
#pragma once
#include <stdint.h>

struct DropParams {          // what a kernel is handed: the header's wj_dropout_args, with p already turned into (thr, scale)
    uint32_t key0, key1;     // seed low / high
    uint32_t stream_id, call;
    uint32_t thr;            // keep iff draw >= thr
    float scale;             // 65536 / (65536 - thr)
};

struct Draws8 { uint32_t w[4]; };

__host__ __device__ inline Draws8 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Draws8{{c0, c1, c2, c3}};
}

// the eight draws of one group
__host__ __device__ inline Draws8 drop_draws(const DropParams& d, uint64_t group) {
    return philox4x32_10((uint32_t)group, (uint32_t)(group >> 32), d.stream_id, d.call, d.key0, d.key1);
}
__host__ __device__ inline uint32_t drop_draw(const Draws8& r, int j) { return (r.w[j >> 1] >> (16 * (j & 1))) & 0xffffu; }
// bit j set = element j of the group is kept
__host__ __device__ inline uint32_t drop_keep_bits(const DropParams& d, uint64_t group) {
    const Draws8 r = drop_draws(d, group);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) bits |= (uint32_t)(drop_draw(r, j) >= d.thr) << j;
    return bits;
}
// attention: the group of (b * H + h, q, key chunk c of 32, lane group g), and the draw of key k inside it
__host__ __device__ inline uint64_t drop_attn_group(uint64_t bh, int q, int c, int g) { return ((bh * 1024u + (uint32_t)q) * 128u) + (uint32_t)(c * 4 + g); }
__host__ __device__ inline int drop_attn_draw(int k) { return 4 * ((k & 31) >> 4) + (k & 3); }
