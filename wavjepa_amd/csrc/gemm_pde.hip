// Persistent bf16 GEMM with a DEFERRED epilogue (variant 6 of wj_gemm_bf16): C[M,N] = gelu(A[M,K] . B[N,K]^T + bias), row-form operands,
// K % 128 == 0, K >= 256, N % 256 == 0, M >= 128; epilogues BIAS_GELU (teacher linear1), BIAS_GELU2 (student / predictor linear1: gelu and
// gelu'), CONV_GELU (sparse conv layers: pre-activation and GELU, rows outside the active segments zeroed).
//
// Why.  In the persistent 256 x 256 kernel (csrc/gemm_persist.hip) an erf-GELU epilogue is pure vector arithmetic -- 14 issue slots per
// output, 18-21 with gelu' -- during which the matrix pipe idles, and the K loop is pure matrix work during which the vector pipe idles:
// 7 us of a 29.5-us item on the teacher's linear1 (K = 768), 13 of 22.4 on the predictor's (K = 384).  All eight waves of a workgroup
// walk in lockstep (they share the staged operand tiles), so the two never overlap, and the 128 accumulators + 64 fragment registers of
// a 128 x 64 wave tile leave no room to keep a finished tile around.  Here the work item is 128 x 256 (wave tile 64 x 64: 64 accumulators):
//   * at the end of an item the accumulators (bias included: it was the C operand of their first MFMA) are rounded to bf16 -- the value
//     GELU is taken of, as nn.GELU sees a bf16 linear's output -- and PARKED, packed, in 32 registers; the K loop of the next item starts
//     at once;
//   * the parked tile is finished in four blocks of 16 rows, one per K tile of the next item's first four K tiles, each inside the load
//     segment of that K tile's second phase: GELU, one trip through the wave's LDS strip (MFMA layout -> whole 128-B lines, as in
//     gemm_persist.hip), 16-byte non-temporal stores.  While one wave group does that, the other runs its MFMA cluster, and vice versa;
//   * the stores sit INSIDE the K-tile stream, between LDS-DMA instructions that share their in-order vmcnt counter: every wait counts
//     them exactly (stores of this K tile and of the previous one are younger than the pieces the wait retires; a store acknowledgement
//     takes ~4 us under load, waiting for one by accident costs more than the block);
//   * K tile = two phases (X x B0, X x B1), three pieces (X: 128 A rows; B0 / B1: the two 32-row halves of every wave column), two LDS
//     parities of 48 KB; piece schedule: B1(t+1) in phase 0 of K tile t, X(t+2) and B0(t+2) in phase 1 (into the parity whose X / B0
//     were read one barrier pair earlier);
//   * tiles are pulled from the per-XCD counters of gemm_persist.hip (same counter sets, same mailbox protocol); edge panels are shifted
//     inwards (M - 128), never clipped.
#include "gemm_pieces.h"
#include "gemm_internal.h"

namespace {

constexpr unsigned BUF = 49152u, BOFF = 16384u;   // LDS: two parities of [A 128 rows | B 256 rows] x 128 B
typedef PersistLds<2u * BUF> L;                   // bias slots, mailbox and the blocks' strips behind the ring, as in gemm_persist.hip
constexpr unsigned AUX = L::AUX, MAILBOX = L::MAILBOX, STAGE = L::STAGE;
constexpr int LDS_TOTAL = L::TOTAL;

struct DArgs : RowArgs {
    unsigned* ctr;
    int ntiles, items_n, wpx;
    int diag;                 // lab build (WJ_PDE_DIAG): bit 0 = never park a tile (the raw K loop: no GELU, no stores, wrong results)
};

template <int EPI> struct Outs {
    static constexpr int N = epi_outputs(EPI);
    static constexpr int S = N * strip_stores(false);   // global stores one wave issues per block of the parked tile
};

// the parked tile of one wave: bf16(acc + bias) of its 64 x 64 outputs in the MFMA layout, and where it goes
struct Parked {
    u32x2 h[4][4];      // [mi][ni]: columns 4 g .. 4 g + 3 of rows mi * 16 + i  (i = lane & 15, g = lane >> 4)
    char* c1;           // C  + this lane's first store address (row srow of block 0, 16-B chunk schunk of the wave's 128-B line)
    char* c2;           // C2 likewise (two-output epilogues)
    int rem;            // CONV_GELU: (row of this lane in block 0) % seg_rows
};

// One 16-row block of the parked tile: GELU, through the strip, stores.  Issues exactly Outs<EPI>::S global stores.
template <int EPI, int MI>
__device__ __forceinline__ void parked_block(const Parked& pk, const StripLane& sl, long ldc_b, int seg_rows, int seg_valid) {
    bool valid = true;
    if constexpr (EPI == WJ_EPI_CONV_GELU) {
        int r = pk.rem + 16 * MI;                    // seg_rows > 16: at most MI wraps
#pragma unroll
        for (int x = 0; x < MI; ++x) r = r >= seg_rows ? r - seg_rows : r;
        valid = r < seg_valid;
    }
    u32x2 o1[4], o2[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const unsigned w0 = pk.h[MI][ni][0], w1 = pk.h[MI][ni][1];
        f32x2 h[2], gl[2], gp[2];
        h[0] = f32x2{__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u)};
        h[1] = f32x2{__uint_as_float(w1 << 16), __uint_as_float(w1 & 0xffff0000u)};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if constexpr (EPI == WJ_EPI_BIAS_GELU2) gelu_pk<true>(h[q], gl[q], gp[q]);
            else gelu_pk<false>(h[q], gl[q], gp[q]);
        }
        u32x2 og = u32x2{pack_bf16(gl[0].x, gl[0].y), pack_bf16(gl[1].x, gl[1].y)};
        if constexpr (EPI == WJ_EPI_BIAS_GELU) {
            o1[ni] = og;
        } else if constexpr (EPI == WJ_EPI_BIAS_GELU2) {
            o1[ni] = u32x2{pack_bf16(gp[0].x, gp[0].y), pack_bf16(gp[1].x, gp[1].y)};   // C  = gelu'(h)
            o2[ni] = og;                                                                   // C2 = gelu(h)
        } else {                                                                           // CONV_GELU: C = pre, C2 = post
            o1[ni] = u32x2{valid ? w0 : 0u, valid ? w1 : 0u};
            o2[ni] = u32x2{valid ? og[0] : 0u, valid ? og[1] : 0u};
        }
    }
    const long off = (long)(MI * 16) * ldc_b;
    const long row8 = 8 * ldc_b;
    strip_store(o1, sl, pk.c1 + off, row8);
    if constexpr (Outs<EPI>::N == 2) strip_store(o2, sl, pk.c2 + off, row8);
}

// One K tile (64 deep) of the stream = two phases.
//   TOP:      first K tile of an item: every accumulator's first MFMA takes the bias as C; top_n VMEM operations were issued in front of it
//             (the NEXT item's bias DMA; in wave 0 also the pull)
//   BLK:      0-3: this K tile carries block BLK of the parked tile (in phase 1's load segment); -1: none
//   prev_s:   global stores the PREVIOUS K tile issued (its block, behind that K tile's LDS-DMAs): younger than the pieces both phases wait for
//   stage_b1: B1(t+1) exists (false only in the last K tile of a workgroup's last item); sw_b1: it is the next item's first
//   stage_x:  X(t+2), B0(t+2) exist (false only in the last two K tiles of the last item); sw_x: they are the next item's first
template <int PAR, bool TOP, int BLK, int EPI>
__device__ __forceinline__ void kstep(f32x4 (&acc)[4][4], char* smem, Bases& s, const char* nA, const char* nB, unsigned b1_full,
                                      const unsigned (&vx)[2], const unsigned (&vb)[2], const unsigned (&dx)[2], const unsigned (&db)[2],
                                      unsigned a_lo, unsigned b_lo, bool sw_b1, bool stage_b1, bool sw_x, bool stage_x, int prev_s,
                                      int top_n, const f32x4 (&bv)[4], const Parked& pk, const StripLane& sl, const DArgs& a, bool mail,
                                      const unsigned& pv) {
    constexpr unsigned CUR = PAR * BUF, OTH = (PAR ^ 1) * BUF;
    constexpr int S = BLK >= 0 ? Outs<EPI>::S : 0;
    char* cur = smem + CUR;
    const unsigned a_hi = a_lo ^ 64u, b_hi = b_lo ^ 64u;
    bf16x8 af[8], b0f[4], b1f[4];
    // ---- phase 0: X, B0 of this K tile; stage B1(t+1) into the other parity; wait for B1(t)
    __builtin_amdgcn_sched_barrier(0);
    read_frags<2>(b0f, cur, b_lo, b_hi);
    read_frags<4>(af, cur, a_lo, a_hi);
    if (stage_b1) {
        if (sw_b1) s.b1 = nB + b1_full;
        dma<OTH + BOFF + 4096>(vb[0], s.b1, db[0]); dma<OTH + BOFF + 4096>(vb[1], s.b1, db[1]);
        s.b1 += 128;
        // younger than B1(t): X(t+1), B0(t+1) (4), the previous K tile's block stores, what went out in front of a first K tile, B1(t+1) (2)
        wait_cnt(6 + prev_s + (TOP ? top_n : 0));
    } else {
        wait_cnt(0);
    }
    phase_mfma<Bf16Mma, 0, 0, TOP>(acc, b0f, af, bv);
    // ---- phase 1: B1 of this K tile; stage X(t+2), B0(t+2) into THIS parity; the parked tile's block; wait for X(t+1), B0(t+1)
    __builtin_amdgcn_sched_barrier(0);
    read_frags<2>(b1f, cur, b_lo + 4096, b_hi + 4096);
    if (stage_x) {
        if (sw_x) { s.x = nA; s.b0 = nB; }
        dma<CUR>(vx[0], s.x, dx[0]); dma<CUR>(vx[1], s.x, dx[1]);
        dma<CUR + BOFF>(vb[0], s.b0, db[0]); dma<CUR + BOFF>(vb[1], s.b0, db[1]);
        s.x += 128; s.b0 += 128;
    }
    if constexpr (BLK >= 0) parked_block<EPI, BLK>(pk, sl, a.ldc_b, a.seg_rows, a.seg_valid);
    __builtin_amdgcn_sched_barrier(0);
    if (stage_x) {
        // younger than X(t+1), B0(t+1): the previous K tile's block stores, what went out in front of a first K tile, B1(t+1) (2), X(t+2),
        // B0(t+2) (4), this block's stores
        wait_cnt(6 + S + prev_s + (TOP ? top_n : 0));
    } else {
        wait_cnt(0);
    }
    if (mail) {
        // the pull went out in front of this item's first K tile: 13 younger operations + two blocks' stores by now, 6 + two blocks' stores in flight
        mailbox_write(pv, MAILBOX);
    }
    phase_mfma<Bf16Mma, 0, 2, TOP>(acc, b1f, af, bv + 2);
}

template <int EPI>
__global__ __launch_bounds__(GEMM_NT, 1) void gemm_pde_kernel(DArgs a) {
    constexpr int S = Outs<EPI>::S;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int n = a.K >> 6;                           // K tiles per item (even, >= 4)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

    // ---- this workgroup's queue: the logical item ids [cstart, cstart + clen) of its XCD label
    const int xl = blockIdx.x & 7;
    const XcdRun run = xcd_run(a.ntiles, xl);
    const int clen = run.len, cstart = run.start;
    if ((int)(blockIdx.x >> 3) >= clen) return;
    unsigned* ctr = a.ctr + xl * CTR_STRIDE;
    unsigned pv = 0;
    auto pull = [&]() {
        if (wave == 0) pull_atomic(pv, ctr);
    };

    // ---- piece geometry of this wave: two 1-KiB instructions (8 rows x 128 B) per piece
    unsigned dx[2], db[2], vx[2], vb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rx = 16 * wave + 8 * u, rb = piece_row_b(wave, u);      // X: the item's 128 A rows, 16 per wave
        dx[u] = lds0 + (unsigned)rx * 128u;
        db[u] = lds0 + (unsigned)rb * 128u;
        vx[u] = piece_voff(rx, lane, a.lda_b);
        vb[u] = piece_voff(rb, lane, a.ldb_b);
    }
    const unsigned b1_full = 32u * a.ldb_b;
    auto item_coords = [&](int q, int& m0, int& n0) {
        const int L = cstart + q;
        const int tm = L / a.items_n;
        m0 = min(tm * 128, a.M - 128);                 // the last panel is shifted inwards
        n0 = (L - tm * a.items_n) * 256;
    };
    const char* bias_src = a.bias ? reinterpret_cast<const char*>(a.bias) : reinterpret_cast<const char*>(g_zero_page);
    auto bias_dma = [&](int n0, int slot) {
        const int ln = opaque(lane);
        const unsigned bias_v = a.bias ? (unsigned)((wn * 64 + (ln & 15) * 4) * 4) : (unsigned)((ln & 15) * 16);
        const char* sb = a.bias ? bias_src + (long)n0 * 4 : bias_src;
        const unsigned dst = lds0 + AUX + (unsigned)(slot * 2048 + wave * 256);
        asm volatile("s_mov_b32 m0, %2\n\ts_mov_b64 exec, 0xffff\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\ts_mov_b64 exec, -1"
                     ::"v"(bias_v), "s"(sb), "s"(dst) : "memory", "m0");
    };

    f32x4 acc[4][4];

    // ---- prologue: the first item is static; pull the second
    int m0, n0;
    item_coords(blockIdx.x >> 3, m0, n0);
    Bases s;
    s.x = a.A + (long)m0 * a.lda_b;
    s.b0 = a.B + (long)n0 * a.ldb_b;
    s.b1 = s.b0 + b1_full;
    bias_dma(n0, 0);
    pull();
    dma<0>(vx[0], s.x, dx[0]); dma<0>(vx[1], s.x, dx[1]);
    dma<BOFF>(vb[0], s.b0, db[0]); dma<BOFF>(vb[1], s.b0, db[1]);
    dma<BOFF + 4096>(vb[0], s.b1, db[0]); dma<BOFF + 4096>(vb[1], s.b1, db[1]);
    s.x += 128; s.b0 += 128; s.b1 += 128;
    dma<BUF>(vx[0], s.x, dx[0]); dma<BUF>(vx[1], s.x, dx[1]);
    dma<BUF + BOFF>(vb[0], s.b0, db[0]); dma<BUF + BOFF>(vb[1], s.b0, db[1]);
    s.x += 128; s.b0 += 128;
    wait_cnt(4);                                       // K tile 0's pieces, the bias and the pull (all older) have landed
    if (wave == 0) mailbox_write(pv, MAILBOX);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    unsigned mail_v = lds_read_u32(MAILBOX);
    mail_v = __builtin_amdgcn_readfirstlane(mail_v);
    if (mail_v == (unsigned)(clen - 1) && t == 0) atomicExch(ctr, 0u);   // the launch's last pull on this counter: reset it
    int q_next = a.wpx + (int)mail_v;
    bool has_next = q_next < clen;

    const unsigned a_lo = frag_off(wm * 64, lane), b_lo = BOFF + frag_off(wn * 64, lane);
    // the strip of this wave, in the MFMA layout (write side) and in the store layout (read side)
    const int ln = opaque(lane);
    StripLane sl;
    sl.init(smem + STAGE + wave * (16 * STRIP_ROW), ln, false);
    const long lane_off = (long)sl.srow * a.ldc_b + (long)(wn * 128 + sl.schunk * 16);

    if (wm == 1) __builtin_amdgcn_s_barrier();        // waves 4-7 run one barrier behind

    Parked pk;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) pk.h[mi][ni] = u32x2{0u, 0u};
    pk.c1 = a.C; pk.c2 = a.C2; pk.rem = 0;
    bool have_parked = false;
    int slot = 0;
    int last_s = 0;                                    // stores issued by the last K tile of the previous item (n == 4 only)
    for (;;) {
        int m1 = m0, n1 = n0;
        const bool pulled = has_next;
        const char* nA = a.A;
        const char* nB = a.B;
        if (has_next) {
            item_coords(q_next, m1, n1);
            nA = a.A + (long)m1 * a.lda_b;
            nB = a.B + (long)n1 * a.ldb_b;
        }
        __builtin_amdgcn_sched_barrier(0);
        bias_dma(n1, slot ^ 1);                        // always exactly one DMA here (the first K tile's waits count it)
        if (pulled) pull();
        __builtin_amdgcn_sched_barrier(0);
        f32x4 bv[4];
        {
            const int g = opaque(lane) >> 4;
            const char* bs = smem + AUX + slot * 2048 + wave * 256;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) bv[ni] = *reinterpret_cast<const f32x4*>(bs + ni * 64 + g * 16);
        }
        const bool hn = has_next;
        const int top_n = (pulled && wave == 0) ? 2 : 1;
        // K tile t: sw_b1 = (t == n - 1), stage_b1 = (t < n - 1 || hn), sw_x = (t + 2 == n), stage_x = (t + 2 < n || hn)
#define KSTEP(PAR, TOP, BLK, T, PREV_S, MAIL)                                                                                                  \
    kstep<PAR, TOP, BLK, EPI>(acc, smem, s, nA, nB, b1_full, vx, vb, dx, db, a_lo, b_lo, (T) == n - 1, (T) < n - 1 || hn, (T) + 2 == n,     \
                              (T) + 2 < n || hn, PREV_S, top_n, bv, pk, sl, a, MAIL, pv)
        if (have_parked) {
            KSTEP(0, true, 0, 0, last_s, false);
            KSTEP(1, false, 1, 1, S, pulled && wave == 0);
            KSTEP(0, false, 2, 2, S, false);
            KSTEP(1, false, 3, 3, S, false);
        } else {
            KSTEP(0, true, -1, 0, 0, false);
            KSTEP(1, false, -1, 1, 0, pulled && wave == 0);
            KSTEP(0, false, -1, 2, 0, false);
            KSTEP(1, false, -1, 3, 0, false);
        }
        int prev = have_parked ? S : 0;
        for (int kt = 4; kt < n; kt += 2) {
            KSTEP(0, false, -1, kt, prev, false);
            KSTEP(1, false, -1, kt + 1, 0, false);
            prev = 0;
        }
#undef KSTEP
        last_s = (n == 4 && have_parked) ? S : 0;
        // ---- park the item: bf16(acc) in the MFMA layout, and where its blocks go
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");     // MFMA results of the last phase -> VALU readers behind the loop branch
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const f32x4 v = acc[mi][ni];
                pk.h[mi][ni] = u32x2{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
            }
        {
            const long tile_off = (long)(m0 + wm * 64) * a.ldc_b + (long)n0 * 2;
            pk.c1 = a.C + tile_off + lane_off;
            if constexpr (Outs<EPI>::N == 2) pk.c2 = a.C2 + tile_off + lane_off;
            if constexpr (EPI == WJ_EPI_CONV_GELU) pk.rem = (m0 + wm * 64 + (ln & 15)) % a.seg_rows;
        }
        have_parked = !(WJ_LAB_BUILD && (a.diag & 1));
        __builtin_amdgcn_sched_barrier(0);
        if (!has_next) break;
        m0 = m1; n0 = n1;
        slot ^= 1;
        if (pulled) {
            unsigned mv = lds_read_u32(MAILBOX);
            mv = __builtin_amdgcn_readfirstlane(mv);
            if (mv == (unsigned)(clen - 1) && t == 0) atomicExch(ctr, 0u);
            q_next = a.wpx + (int)mv;
            has_next = q_next < clen;
        }
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();        // balance the stagger
    // ---- the last item's parked tile: nothing left to hide it under
    if (WJ_LAB_BUILD && (a.diag & 1)) return;
    parked_block<EPI, 0>(pk, sl, a.ldc_b, a.seg_rows, a.seg_valid);
    parked_block<EPI, 1>(pk, sl, a.ldc_b, a.seg_rows, a.seg_valid);
    parked_block<EPI, 2>(pk, sl, a.ldc_b, a.seg_rows, a.seg_valid);
    parked_block<EPI, 3>(pk, sl, a.ldc_b, a.seg_rows, a.seg_valid);
}

template <int EPI>
int launch_pde(const wj_gemm_args* a, hipStream_t s, unsigned* ctr) {
    DArgs p;
    p.set(a);
    p.ctr = ctr;
    p.items_n = a->N / 256;
    p.ntiles = ((a->M + 127) / 128) * p.items_n;
    p.wpx = wj_gemm_persist_wpx(a);
    {
        static const int diag = wj_lab_env_int("WJ_PDE_DIAG", 0);
        p.diag = diag;
    }
    return launch_with_lds<gemm_pde_kernel<EPI>>(dim3(8 * p.wpx), LDS_TOTAL, s, p);
}

}  // namespace

bool wj_gemm_pde_eligible(const wj_gemm_args* a) {
    if (!row_form_common_ok(a, 128, 256) || a->colsum || a->aux || ((uintptr_t)a->C2 & 15)) return false;
    if (a->K < 256 || (a->K % 128) || a->M < 128 || a->N < 256 || (a->N % 256)) return false;
    const int e = a->epilogue;
    if (e != WJ_EPI_BIAS_GELU2 && e != WJ_EPI_BIAS_GELU && e != WJ_EPI_CONV_GELU) return false;
    if ((e == WJ_EPI_BIAS_GELU2 || e == WJ_EPI_CONV_GELU) && !a->C2) return false;
    if (e == WJ_EPI_CONV_GELU && a->seg_rows > 0 && a->seg_rows <= 16) return false;
    const long items = (long)((a->M + 127) / 128) * (a->N / 256);
    if (items < 512) return false;                    // two rounds of 256 workgroups at least: a parked tile needs a next item to hide under
    return true;
}

int wj_gemm_pde_launch(const wj_gemm_args* a, hipStream_t s) {
    if (!wj_gemm_pde_eligible(a)) return WJ_ERR_UNSUPPORTED;
    unsigned* ctr = wj_gemm_persist_counters(s, nullptr);
    if (!ctr) return WJ_ERR_UNSUPPORTED;
    switch (a->epilogue) {
        case WJ_EPI_BIAS_GELU2: return launch_pde<WJ_EPI_BIAS_GELU2>(a, s, ctr);
        case WJ_EPI_BIAS_GELU: return launch_pde<WJ_EPI_BIAS_GELU>(a, s, ctr);
        case WJ_EPI_CONV_GELU: return launch_pde<WJ_EPI_CONV_GELU>(a, s, ctr);
        default: return WJ_ERR_UNSUPPORTED;
    }
}
