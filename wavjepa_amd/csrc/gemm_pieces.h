// The pieces the dense-contraction kernels are made of, one copy each: csrc/gemm.hip (one tile per workgroup: plain, ping-pong and
// eight-phase schedules, MX fp8), csrc/gemm_persist.hip (persistent eight-phase), csrc/gemm_pde.hip (persistent, deferred epilogue) and
// csrc/gemm_panel.hip (row panels) include this header; what is left in each file is its own staging and wait logic -- the schedule.
//   helpers   : u32x2 / u32x4, opaque, wait_vmcnt, wait_cnt, pack_bf16, store16, lds_read_u32, dma (scalar-base LDS-DMA), pull_atomic,
//               mailbox_write, g_zero_page, Bases, PersistLds, CTR_STRIDE
//   geometry  : swz128, piece_voff, frag_off, piece_row_x / piece_row_b, xcd_run
//   K tile    : read_frags, Bf16Mma / MxMma, mfma_cluster, phase_mfma
//   epilogue  : StripLane, strip_transpose, strip_store, strip_stores / epi_outputs (the VMEM operations the vmcnt arithmetic counts)
// The host pieces (launch_with_lds, row_form_common_ok, RowArgs) are in gemm_internal.h.
#pragma once
#include "common.h"
#include "../../include/wavjepa_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef int v8i32 __attribute__((ext_vector_type(8)));
typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gl_void;

// K tails / out-of-range columns of the one-tile kernels read this page instead of being predicated; the persistent kernels stage it as
// the bias of a call without one.
__device__ __attribute__((aligned(256))) unsigned char g_zero_page[256];

constexpr int GEMM_NT = 512;                      // threads per workgroup of every MFMA kernel here: 8 waves
constexpr int CTR_STRIDE = 32;                    // dwords between the 8 tile counters of a set (one 128-B line each)
constexpr unsigned STRIP_ROW = 144u;              // 128 B of bf16 + 16: the 8-byte writes of a 32-lane pass and the 16-byte reads of a row hit distinct banks

// LDS of the persistent kernels behind their operand ring of RING bytes
template <unsigned RING> struct PersistLds {
    static constexpr unsigned AUX = RING;                 // [2 items][8 waves][64 floats] bias of the wave's 64 columns
    static constexpr unsigned MAILBOX = AUX + 4096u;      // next-next item index, written by wave 0
    static constexpr unsigned STAGE = MAILBOX + 256u;     // [8 waves][16 rows x STRIP_ROW B]: the epilogue's transpose (per wave, no barriers)
    static constexpr int TOTAL = (int)(STAGE + 8u * 16u * STRIP_ROW);
};

// wave-uniform source bases of the next LDS-DMA of each piece (X = A rows 0-63 of each wave row, Y = rows 64-127, B0 = B rows
// 0-31 of each wave column, B1 = rows 32-63), advanced by 128 B per K tile
struct Bases {
    const char* x;
    const char* y;
    const char* b0;
    const char* b1;
};

// A value hipcc cannot relate to its source: address arithmetic built on it is redone where it is written instead of being
// hoisted out of the tile loop and kept in registers across the MFMA phases (the loop runs at 128 accumulators + 64 fragment
// registers per lane; hoisted tables spill to scratch, and every scratch access is a vmcnt(0) in the LDS-DMA ring).
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_waitcnt vmcnt(n), n a run-time value in 0..16 (thresholds that depend on what else shares the in-order counter)
__device__ __forceinline__ void wait_cnt(int n) {
    switch (n) {
        case 0: wait_vmcnt<0>(); break;
        case 1: wait_vmcnt<1>(); break;
        case 2: wait_vmcnt<2>(); break;
        case 3: wait_vmcnt<3>(); break;
        case 4: wait_vmcnt<4>(); break;
        case 5: wait_vmcnt<5>(); break;
        case 6: wait_vmcnt<6>(); break;
        case 7: wait_vmcnt<7>(); break;
        case 8: wait_vmcnt<8>(); break;
        case 9: wait_vmcnt<9>(); break;
        case 10: wait_vmcnt<10>(); break;
        case 11: wait_vmcnt<11>(); break;
        case 12: wait_vmcnt<12>(); break;
        case 13: wait_vmcnt<13>(); break;
        case 14: wait_vmcnt<14>(); break;
        case 15: wait_vmcnt<15>(); break;
        default: wait_vmcnt<16>(); break;
    }
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    bf16x2 p;
    p[0] = f2bf(a);
    p[1] = f2bf(b);
    return __builtin_bit_cast(unsigned, p);
}

// 16-byte non-temporal global store: the C tile is not re-read by this kernel, and kept out of the L2's way its operand panels
// stay resident (measured with tools/persist_stamps.py: 1.30 instead of 1.37 us per K tile on the teacher's QKV shape, and
// 0.6 us less store-acknowledge stall per tile; sc1 / sc0 sc1 write-through forms were slower than plain stores).
__device__ __forceinline__ void store16(char* p, const u32x4& v) {
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
}

// One dword from LDS byte address `addr` (the kernel's only LDS is the dynamic block at 0).  From asm: a `volatile` C++ read of the mailbox is
// not rewritten to the LDS address space by hipcc -- it became a FLAT load, and a flat load is waited for with vmcnt(0): every item boundary
// drained the epilogue's stores and the staged LDS-DMA pieces that the counted waits of the next K tiles are there to leave in flight
// (found in round 6 in the ISA of the round-3 kernel).
__device__ __forceinline__ unsigned lds_read_u32(unsigned addr) {
    unsigned v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}

// One LDS-DMA instruction with SCALAR addressing: 64 lanes x 16 B from sbase + voff (voff: a per-lane constant of the kernel, sbase: a
// wave-uniform SGPR pair advanced by the scalar unit) to LDS bytes [lds_wave + LDS_CONST + 16 lane).  M0 is written here and nowhere
// else in the kernels that use it (no builtin LDS-DMA is left in them).  Two emitted forms: with a compile-time constant (the parities and
// pieces of the persistent kernels' rings, 0 included) `s_add_u32 m0, lds_wave, LDS_CONST`; without one (the panel's run-time slots)
// `s_mov_b32 m0, lds_wave`.  (The one-tile kernels of gemm.hip keep per-lane 64-bit pointers and the builtin: a measured design point.)
constexpr unsigned DMA_NO_CONST = ~0u;
template <unsigned LDS_CONST = DMA_NO_CONST>
__device__ __forceinline__ void dma(unsigned voff, const char* sbase, unsigned lds_wave) {
    if constexpr (LDS_CONST == DMA_NO_CONST)
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_wave) : "memory", "m0");
    else
        asm volatile("s_add_u32 m0, %2, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                     ::"v"(voff), "s"(sbase), "s"(lds_wave), "n"(LDS_CONST) : "memory", "m0", "scc");
}

// The pull of a persistent kernel's next item, by lane 0 of the calling wave: pv = (*ctr)++.  A returning atomic from inline asm: its
// result register is not tracked by hipcc's waitcnt pass (a tracked one would drain the LDS-DMA ring with vmcnt(0) at first use); it is
// consumed, again from asm (mailbox_write), behind a counted wait that covers it (tools/asm_checks.py verifies that nothing touches
// the register in between).
__device__ __forceinline__ void pull_atomic(unsigned& pv, unsigned* ctr) {
    asm volatile("s_mov_b64 exec, 1\n\ts_nop 0\n\tglobal_atomic_add %0, %1, %2, %3 sc0\n\ts_mov_b64 exec, -1"
                 : "+v"(pv) : "v"(0u), "v"(1u), "s"(ctr) : "memory");
}
// ... and its hand-over to the other waves: lane 0 writes pv to the LDS word at byte `mailbox`
__device__ __forceinline__ void mailbox_write(const unsigned& pv, unsigned mailbox) {
    asm volatile("s_mov_b64 exec, 1\n\ts_nop 0\n\tds_write_b32 %1, %0\n\ts_mov_b64 exec, -1\n\ts_waitcnt lgkmcnt(0)"
                 ::"v"(pv), "v"(mailbox) : "memory");
}

// ---- geometry of the 128-byte-row LDS image (64 bf16 / 128 fp8 of k per row) ----------------------------------------------------
// 16-B chunk c of row r sits at chunk position c ^ ((r >> 1) & 7): conflict-free for the ds_read_b128 lane groups.  The swizzle is
// applied to the per-lane SOURCE address of the LDS-DMA (the image itself is lane-linear: what LDS-DMA can write) and again on the read.
__device__ __forceinline__ int swz128(int chunk, int row) { return chunk ^ ((row >> 1) & 7); }

// One LDS-DMA instruction covers 8 rows x 128 B: lane -> (row r0 + lane / 8, LDS chunk position lane % 8).  Per-lane source bytes
// relative to the tile origin, rows ld_b bytes apart.
__device__ __forceinline__ unsigned piece_voff(int r0, int lane, unsigned ld_b) {
    const int row = r0 + (lane >> 3);
    return (unsigned)row * ld_b + (unsigned)(swz128(lane & 7, row) * 16);
}

// Fragment read offset inside an operand region: lane (i, g) = (lane & 15, lane >> 4) reads row row0 + i (row0 % 16 == 0), chunk g
// (k 0-31) here and chunk g ^ 4 (k 32-63) at this offset ^ 64; the further 16-row blocks are 2048 B apart (read_frags).
__device__ __forceinline__ unsigned frag_off(int row0, int lane) {
    const int i = lane & 15, g = lane >> 4;
    return (unsigned)((row0 + i) * 128) + (unsigned)(swz128(g, i) << 4);
}

// First tile row of instruction u (0 / 1) of this wave's share of a piece.  X of a 256-row A tile: rows 0-63 of wave row 0 (waves 0-3)
// / 1 (waves 4-7), Y = X + 64 rows; B0: rows 0-31 of each wave column, the waves pair up on a column, B1 = B0 + 32 rows.
__device__ __forceinline__ int piece_row_x(int wave, int u) { return (wave < 4 ? 16 * wave : 128 + 16 * (wave - 4)) + 8 * u; }
__device__ __forceinline__ int piece_row_b(int wave, int u) {
    const int ib = 16 * wave + 8 * u;
    return (ib >> 5) * 64 + (ib & 31);
}

// The contiguous run of n work items that XCD label xl (workgroup id % 8: round-robin dispatch) owns, as xcd_remap deals them
struct XcdRun { int start, len; };
__device__ __forceinline__ XcdRun xcd_run(int n, int xl) {
    const int q = n >> 3, r = n & 7;
    XcdRun x;
    x.len = q + (xl < r ? 1 : 0);
    x.start = xl < r ? xl * (q + 1) : r * (q + 1) + (xl - r) * q;
    return x;
}

// ---- the pieces of a K-tile phase ---------------------------------------------------------------------------------------------
// N 16-row blocks of fragments: f[2 x] = chunk g, f[2 x + 1] = chunk g ^ 4 of row block x (lo = frag_off(..), hi = lo ^ 64)
template <int N, class T>
__device__ __forceinline__ void read_frags(T* f, const char* cur, unsigned lo, unsigned hi) {
#pragma unroll
    for (int x = 0; x < N; ++x) {
        f[2 * x] = *reinterpret_cast<const T*>(cur + lo + x * 2048);
        f[2 * x + 1] = *reinterpret_cast<const T*>(cur + hi + x * 2048);
    }
}

// The builtin form of the scaled MFMA is allocated with a destination DISTINCT from its accumulator input (early-clobber), which
// at 128 accumulator registers per lane spills ~150 of them to scratch (and every scratch access is a vmcnt(0) in the LDS-DMA
// ring).  In hardware vdst == srcC is the ordinary accumulate form, so the instruction is written out with the two tied.
// "s_nop 1": VALU-written scale registers feed the MFMA (hipcc pads nothing inside an asm statement).
__device__ __forceinline__ void mx_mfma(f32x4& acc, const v8i32& a, const v8i32& b, int scale_a, int scale_b) {
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(scale_a), "v"(scale_b));
}

// The product of one 16 x 16 output fragment with one K tile, from the two 16-B chunks (b[0], b[1]) / (a[0], a[1]) of its operand rows.
// Operands are swapped (B first) so that a lane owns 4 consecutive output columns.
struct Bf16Mma {              // 64 bf16 of k: two v_mfma_f32_16x16x32_bf16, the first one on C = c (the accumulator, or the bias)
    typedef bf16x8 Chunk;
    static __device__ __forceinline__ void mma(f32x4& acc, const f32x4& c, const Chunk* b, const Chunk* a, int, int) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[0], a[0], c, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[1], a[1], acc, 0, 0, 0);
    }
};
struct MxMma {                // 128 e4m3 of k: the two chunks are the halves of ONE block-scaled operand
    typedef v4i32 Chunk;
    static __device__ __forceinline__ void mma(f32x4& acc, const f32x4&, const Chunk* b, const Chunk* a, int sb, int sa) {
        mx_mfma(acc, __builtin_shufflevector(b[0], b[1], 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(a[0], a[1], 0, 1, 2, 3, 4, 5, 6, 7), sb, sa);
    }
};

// The 4 x 2 MFMA cluster of one phase: accumulator quadrant acc[MI0 .. MI0 + 3][NI0 .. NI0 + 1] += A row blocks af[2 mi], af[2 mi + 1] x
// B row blocks bfr[2 ni], bfr[2 ni + 1], at raised priority.  CINIT: the first MFMA of every accumulator takes c0[ni] as C instead of the
// accumulator (the bias of the persistent kernels: no clearing, no bias add in the epilogue).  sb / sa: the MX block scales per row block.
template <class OP, int MI0, int NI0, bool CINIT = false, int R, int C>
__device__ __forceinline__ void mfma_cluster(f32x4 (&acc)[R][C], const typename OP::Chunk* bfr, const typename OP::Chunk* af,
                                             const f32x4* c0 = nullptr, const int* sb = nullptr, const int* sa = nullptr) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            OP::mma(acc[MI0 + mi][NI0 + ni], CINIT ? c0[ni] : acc[MI0 + mi][NI0 + ni], bfr + 2 * ni, af + 2 * mi, sb ? sb[ni] : 0, sa ? sa[mi] : 0);
    __builtin_amdgcn_s_setprio(0);
}

// The compute half of a phase of the eight-phase schedules: the barrier that ends the load half (every wave's fragment reads and
// LDS-DMA issue), the cluster, the barrier that ends the phase.  skip: a half-width item leaves the B1 quadrants out, barriers stay.
template <class OP, int MI0, int NI0, bool CINIT = false, int R, int C>
__device__ __forceinline__ void phase_mfma(f32x4 (&acc)[R][C], const typename OP::Chunk* bfr, const typename OP::Chunk* af,
                                           const f32x4* c0 = nullptr, const int* sb = nullptr, const int* sa = nullptr, bool skip = false) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (!skip) mfma_cluster<OP, MI0, NI0, CINIT>(acc, bfr, af, c0, sb, sa);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
}

// ---- per-wave strip epilogue ----------------------------------------------------------------------------------------------------
// In the MFMA layout consecutive lanes hold different ROWS, and a wave store whose consecutive lanes touch different cache lines is handled
// line by line: 2.3 us per 128-KB tile and CU however the lanes are permuted inside the wave, against 0.6 us when every 8 consecutive
// lanes write one whole 128-B line (tools/micro/store_path.hip).  So each 16-row block of bf16 outputs takes one trip through a per-wave
// LDS strip of 16 rows x STRIP_ROW bytes: NI 8-byte writes in the MFMA layout (lane (i, g): row i, columns 16 ni + 4 g .. + 3), then
//   full width (NI = 4): two 16-byte reads with lane -> (row lane >> 3 [+ 8], 16-B chunk lane & 7), two stores of 8 rows x 128 B;
//   half width (NI = 2): one read with lane -> (row lane >> 2, chunk lane & 3), one store of 16 rows x 64 B.
// One wave's LDS operations execute in order, so the strip needs neither waits nor barriers between its uses.
struct StripLane {
    char* wr;            // this lane's write address (+ ni * 32)
    const char* rd;      // this lane's read address (+ 8 * STRIP_ROW for rows 8-15, full width)
    int srow, schunk;    // the row (of the block's first 8 / 16) and the 16-B chunk this lane stores
    __device__ __forceinline__ void init(char* strip, int ln, bool half) {
        wr = strip + (ln & 15) * STRIP_ROW + (ln >> 4) * 8;
        srow = half ? (ln >> 2) : (ln >> 3);
        schunk = half ? (ln & 3) : (ln & 7);
        rd = strip + srow * STRIP_ROW + schunk * 16;
    }
};

// global stores one wave issues for ONE 16-row block of ONE output (strip_store); the counted vmcnt waits of the kernels that keep
// stores in flight under their LDS-DMA stream derive their thresholds from this and from epi_outputs
constexpr int strip_stores(bool half) { return half ? 1 : 2; }
// outputs an epilogue writes (C, or C and C2)
constexpr int epi_outputs(int epi) { return (epi == WJ_EPI_BIAS_GELU2 || epi == WJ_EPI_CONV_GELU) ? 2 : 1; }

template <int NI>
__device__ __forceinline__ void strip_transpose(const u32x2 (&o)[NI], const StripLane& sl, u32x4& lo, u32x4& hi) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) *reinterpret_cast<u32x2*>(sl.wr + ni * 32) = o[ni];
    // No instruction; keeps the compiler from moving the strip's writes / reads across these points.  The lanes exchange data
    // through the strip without a barrier hipcc knows of: with a branch around the stores (tried for half-width tiles) it sank the
    // second output's strip WRITES into the branch -- in one thread's view their only reader -- and the lanes outside never wrote.
    __builtin_amdgcn_wave_barrier();
    lo = *reinterpret_cast<const u32x4*>(sl.rd);
    if constexpr (NI == 4) hi = *reinterpret_cast<const u32x4*>(sl.rd + 8 * STRIP_ROW);
    __builtin_amdgcn_wave_barrier();
}

// write, wave_barrier, read, wave_barrier, store16: exactly strip_stores(NI == 2) global stores (none with nostore, a lab diagnostic
// that keeps the values alive).  dst: this lane's address in the block's first row group; row8: bytes to the row 8 further down.
template <int NI>
__device__ __forceinline__ void strip_store(const u32x2 (&o)[NI], const StripLane& sl, char* dst, long row8, bool nostore = false) {
    u32x4 lo, hi;
    strip_transpose(o, sl, lo, hi);
    if (nostore) {
        asm volatile("" ::"v"(lo));
        if constexpr (NI == 4) asm volatile("" ::"v"(hi));
        return;
    }
    store16(dst, lo);
    if constexpr (NI == 4) store16(dst + row8, hi);
}

}  // namespace
