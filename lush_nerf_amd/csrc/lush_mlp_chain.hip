// lush-march: register-resident forward chain of the NeRF MLPs for gfx950 (MI355X).
//
// Same function as mlp_fwd_kernel (lush_mlp.hip; utils/run_lushnerf_helpers.py:334-344, 394-423,
// 483-512 and NeRFAll.mlpforward, models/lushnerf.py:234-266) with the operand roles of the on-chip
// memories swapped:
//
//   * a wave owns 32 points for the whole network.  Their activations never leave its registers: the
//     32x32 MFMA accumulator of a layer (rows = features, columns = points) is turned into bf16
//     planes in place and IS the B operand of the next layer.  This works because the contraction
//     index may be permuted freely: the weights are packed with the rows of every 32-row block
//     permuted by chain_row() (lush_mlp.h), so that the 16 accumulators of a lane are the 2 x 8
//     consecutive features that lane supplies for two 16-wide k-blocks.  No activation image in LDS,
//     no ds_write epilogue, no barrier between layers.
//   * the WEIGHTS are the shared operand: one stream of 1-KiB A fragments per network, in consumption
//     order, moved L2 -> LDS by LDS-DMA into a ring of CH_S slots (one k-block of all row blocks per
//     slot) and read by the 4 waves of the workgroup.  128 points share every weight byte: a quarter
//     of the L2 -> CU traffic per point of the 64-point/8-wave kernel, which was co-limiting there
//     (weights streamed at ~45 B/clk/CU against 64 peak while the MFMAs waited).
//
// One wave per SIMD, 512 registers: 128 accumulators + 128 activation-plane registers + A fragments.
// Synchronisation: one raw s_barrier per stream position ("mid-step"), between the two halves of the
// position's MFMAs: it publishes the DMA of the NEXT position (each wave first waits for its own
// pieces with a counted s_waitcnt vmcnt) and frees the slot of the CURRENT one (its second-half
// fragments are already in registers), which is refilled at once with position +CH_S.
#include "lush_common.h"
#include "lush_mlp.h"
#include "lush_mlp_dev.h"
#include "lush_host.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

namespace lush {

constexpr int CH_S = 4;                       // ring slots = prefetch distance in stream positions
constexpr int CH_MT = 128, CH_NW = 4, CH_NT = 256;
enum { B_REG = 0, B_PEX = 1, B_PED = 2 };     // where a phase takes its B operand from

// Stream schedule of one network.  A "position" is what one ring slot holds: G consecutive k-blocks of
// all row blocks of a segment, G chosen so that every position is a multiple of 4 one-KiB pieces
// (each wave issues the same number of DMAs per position, so vmcnt immediates are static).
// Trunk positions (L0 .. L{NL-1}, FEAT) all have the same shape and sit at p * SLOT in the stream;
// the "tail" list is FEAT | ALPHA | VA | VB | RGB | first CH_S positions of the next tile.
template <class N, int NS, bool HAS_ALPHA>
struct ChSched {
    static constexpr int ENTRY = NS * 1024;
    static constexpr int S = CH_S;
    // trunk positions hold GT k-blocks: with one plane a single k-block is only 8 MFMAs per wave, too
    // little to cover the LDS latency of the next half's fragments
    static constexpr int GT = NS == 1 ? 2 : 1;
    static constexpr int TRUNK_PIECES = N::NRB * NS * GT;
    static constexpr int SLOT = TRUNK_PIECES * 1024;
    static constexpr int PT = (N::KKX + (N::NL - 1) * N::KKH + (N::SKIP > 0 ? N::KKX : 0)) / GT;
    static_assert(N::KKX % GT == 0 && N::KKH % GT == 0, "trunk k-blocks must group evenly");
    // narrow segments: as many k-blocks per position as fit a slot (fewer positions = fewer barriers), dividing K
    static constexpr int grp(int nrb, int kk) {
        int g = 1;
        for (int c = 1; c <= kk; ++c)
            if (kk % c == 0 && nrb * NS * c <= TRUNK_PIECES) g = c;
        return g;
    }
    static constexpr int G_A = grp(1, N::KKH), G_VA = grp(N::NRBV, N::KKH), G_VB = grp(N::NRBV, N::KKD), G_R = grp(1, N::KKV);
    static constexpr int NP_F = N::KKH / GT;
    static constexpr int NP_A = HAS_ALPHA ? N::KKH / G_A : 0;
    static constexpr int NP_VA = N::KKH / G_VA, NP_VB = N::KKD / G_VB, NP_R = N::KKV / G_R;
    static constexpr int T_A = NP_F, T_VA = T_A + NP_A, T_VB = T_VA + NP_VA, T_R = T_VB + NP_VB, T_END = T_R + NP_R;
    static_assert(N::fwd_FEAT == PT * N::NRB * GT, "FEAT must follow the trunk in the stream");
    static_assert(TRUNK_PIECES % 4 == 0 && (NS * G_A) % 4 == 0 && (N::NRBV * NS * G_VA) % 4 == 0 && (N::NRBV * NS * G_VB) % 4 == 0 &&
                      (NS * G_R) % 4 == 0, "stream positions must be whole multiples of 4 pieces");
    static_assert(G_A % 2 == 0 && (N::NRBV * G_VA) % 2 == 0 && (N::NRBV * G_VB) % 2 == 0 && G_R % 2 == 0, "a position needs an even number of units");
    static constexpr int tail_pieces(int t) {
        if (t < T_A) return TRUNK_PIECES;
        if (t < T_VA) return NS * G_A;
        if (t < T_VB) return N::NRBV * NS * G_VA;
        if (t < T_R) return N::NRBV * NS * G_VB;
        if (t < T_END) return NS * G_R;
        return TRUNK_PIECES;
    }
    static constexpr unsigned tail_off(int t) {        // bytes from the start of the stream
        if (t < T_A) return (unsigned)(PT + t) * SLOT;
        if (t < T_VA) return (unsigned)N::fwd_ALPHA * ENTRY + (unsigned)(t - T_A) * G_A * ENTRY;
        if (t < T_VB) return (unsigned)N::fwd_VA * ENTRY + (unsigned)(t - T_VA) * (N::NRBV * G_VA) * ENTRY;
        if (t < T_R) return (unsigned)N::fwd_VB * ENTRY + (unsigned)(t - T_VB) * (N::NRBV * G_VB) * ENTRY;
        if (t < T_END) return (unsigned)N::fwd_RGB * ENTRY + (unsigned)(t - T_R) * G_R * ENTRY;
        return (unsigned)(t - T_END) * SLOT;
    }
    // vmcnt that means "my pieces of position t+1 have landed" at the mid-step of tail position t: the
    // DMAs of t+2 .. t+CH_S-1 are younger.  (Other vector-memory operations issued since -- stash and
    // mask stores -- only make the true count larger, i.e. the wait conservative.)
    static constexpr int tail_wait(int t) {
        int n = 0;
        for (int j = 2; j < CH_S; ++j) n += tail_pieces(t + j) / 4;
        return n;
    }
    static constexpr int trunk_wait = (CH_S - 2) * TRUNK_PIECES / 4;
    static constexpr int WRAP = 0;          // trunk positions never wrap: the tail follows them
};

// Row length of the dZv stash: one plane carries DZV_EXT more columns (lush_mlp.h)
template <int NS, int HV>
struct DzvLd { static constexpr int v = HV + (NS == 1 ? DZV_EXT : 0); };

template <int N_>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

struct ChCtx {
    const char* ring;      // LDS ring (generic pointer, for the fragment reads)
    unsigned ring_lds;     // its LDS byte address (DMA destination)
    const char* gbase;     // stream base (wave-uniform)
    int cslot;             // slot of the position being consumed
    unsigned trunk_pos;    // index of the trunk position being consumed
    int w, lane;
    unsigned voff[4];      // per-lane byte offset of this wave's d-th DMA piece of a position: 16*lane + 4096*d + 1024*w
};

// DMA piece d of this wave (d = 0 .. PIECES/4-1) of a position: global bytes [off + (w + 4d) KiB, +1 KiB)
// of the stream -> the same offset inside ring slot `dst`.
template <int PIECES, int SLOT>
__device__ __forceinline__ void ch_issue(const ChCtx& cx, unsigned off, int slot) {
    const unsigned dst = cx.ring_lds + (unsigned)slot * SLOT + (unsigned)cx.w * 1024u;
    const char* src = cx.gbase + off;
#pragma unroll
    for (int d = 0; d < PIECES / 4; ++d) dma16s(src, cx.voff[d], __builtin_amdgcn_readfirstlane(dst + (unsigned)d * 4096u));
}

template <int NS, int NU>
__device__ __forceinline__ void ch_loadA(bf16x8 (&a)[NU][NS], const char* slot, int u0, int lane) {
#pragma unroll
    for (int i = 0; i < NU; ++i)
#pragma unroll
        for (int p = 0; p < NS; ++p)
            a[i][p] = *reinterpret_cast<const bf16x8*>(slot + ((u0 + i) * NS + p) * 1024 + lane * 16);
}

// One segment: acc[rb] += W[rb rows][K] * B[K][this wave's 32 points], K = NPOS * G k-blocks.
// Unit u of a position = (k-block u / NRBS, row block u % NRBS); the position's units are processed
// in two halves around the "mid-step" (counted vmcnt wait + one s_barrier) that publishes the DMA of
// the next position and frees this position's slot.
//
// With ONE wave per SIMD every instruction of the wave costs an issue slot (~4 cycles) and only what
// sits between two MFMAs is hidden (about 5 instructions per 32-cycle MFMA).  So the schedule is
// written out: each MFMA is followed by at most a few "fillers" and pinned with sched_barrier --
//   half 1: fragment reads of half 2 (one per MFMA), then the global stores of a stash job;
//   half 2: the DMAs that refill the freed slot with position +CH_S, interleaved with the fragment
//           reads of the next position's half 1, then the LDS write + read-back of a stash job.
// MFMAs of a half run term by term over its units so consecutive MFMAs hit different accumulators.
//
// Stash (SP > 0: the planes this phase consumes are the previous layer's activations, which the
// backward needs as [plane][point][LD] rows).  A lane holds 16 bytes of a row per k-block, so
// stores straight from registers would write 32-byte pieces.  Instead a "job" = (group of 4
// k-blocks, plane) goes through a 4-KiB per-wave LDS tile [32 rows][128 B] (XOR-swizzled): 4
// ds_write_b128, 4 ds_read_b128 that return 8 rows x 128 B each, 4 global stores of full 128-byte
// row segments.  Wave-private, so LDS ordering alone synchronises it.  Jobs are spread evenly over
// the positions of the phase.
template <class SC, int NS, int DT, int NRBS, int G, int NPOS, int BSRC, bool TRUNK, int T0, int KX, int SP, int LD>
struct ChPhase {
    static constexpr int U = NRBS * G, H = U / 2;
    static_assert(U % 2 == 0, "a position needs an even number of units");
    static_assert(NS == 1 || NS == 2, "chain kernel: 1 or 2 planes");
    static_assert(SP <= NS, "cannot stash more planes than computed");
    static constexpr int PE_PLANE = CH_MT * PE_ROW * 2;
    static constexpr int TERMS = NS == 2 ? 3 : 1;
    static constexpr int NM = H * TERMS;                      // MFMAs per half
    static constexpr int NF = H * NS;                         // fragments per half
    static constexpr int NJOB = SP > 0 ? (NPOS * G / 4) * SP : 0;
    static_assert(SP == 0 || ((NPOS * G) % 4 == 0 && NJOB <= NPOS), "stash jobs must fit the positions of the phase");
    static constexpr int SPACING = NJOB > 0 ? NPOS / NJOB : 1;
    // job whose LDS write + read-back runs in position i (-1: none); its global stores run in position
    // i + 1 when the jobs are at least 2 positions apart, else at the end of the same position
    static constexpr int job_wr(int i) { return (NJOB > 0 && i % SPACING == 0 && i / SPACING < NJOB) ? i / SPACING : -1; }
    static constexpr int job_st1(int i) { return (SPACING >= 2 && i >= 1) ? job_wr(i - 1) : -1; }   // stores in half 1
    static constexpr int job_st2(int i) { return SPACING >= 2 ? -1 : job_wr(i); }                   // stores in half 2
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    // Stash stores this wave has issued AFTER the DMA of position I+1 (issued in half 2 of position I+1-S, ahead of that
    // half's stash fillers) by the time position I reaches its mid-step wait.  vmcnt counts stores and DMAs together in
    // issue order, so the wait must name them: leaving them out turns "position I+1 has landed" into "positions I+1 ..
    // I+S-1 have landed" whenever stores were issued in between, i.e. a wait for DMAs issued only a position ago.  Only
    // stores of THIS phase are counted (an undercount is safe, an overcount would release the wait early).
    static constexpr int st1_at(int i) { return (i >= 0 && i < NPOS && job_st1(i) >= 0) ? 4 : 0; }
    static constexpr int st2_at(int i) { return (i >= 0 && i < NPOS && job_st2(i) >= 0) ? 4 : 0; }
    static constexpr int younger_stores(int I) {
        int n = st2_at(I + 1 - SC::S) + st1_at(I);
        for (int i = I + 2 - SC::S; i < I; ++i) n += st1_at(i) + st2_at(i);
        return n;
    }

    struct Regs {
        bf16x8 a0[H][NS], a1[H][NS];
        bf16x8 bpe[G][NS];
        u32x4 sb[4];
    };
    struct Stash {
        char* tile;            // this wave's 4-KiB LDS tile
        __bf16* rows;          // stash array, at this wave's first point
        long long plane;       // plane stride (elements)
    };

    // MFMA m of a half whose first unit is U0: term-major over the units
    template <int I, int U0, int M>
    static __device__ __forceinline__ void mfma_m(f32x16 (&acc)[NRBS], const bf16x8 (&a)[H][NS], const bf16x8 (&xin)[KX][NS],
                                                  const bf16x8 (&bpe)[G][NS]) {
        constexpr int term = M / H, u = M % H, uu = U0 + u, rb = uu % NRBS, kbl = uu / NRBS;
        constexpr int pa = NS == 2 ? (term == 0 ? 1 : 0) : 0;     // A plane: lo, hi, hi
        constexpr int pb = NS == 2 ? (term == 1 ? 1 : 0) : 0;     // B plane: hi, lo, hi
        const bf16x8& bv = [&]() -> const bf16x8& {
            if constexpr (BSRC != B_REG) return bpe[kbl][pb];
            else return xin[I * G + kbl][pb];
        }();
        if constexpr (DT == DT_F16) acc[rb] = mfma_f16(a[u][pa], bv, acc[rb]);
        else acc[rb] = mfma_bf16(a[u][pa], bv, acc[rb]);
    }

    static __device__ __forceinline__ void st_write(const Stash& st, const bf16x8 (&xin)[KX][NS], int job, int kq, int lane) {
        const int n = lane & 31, hh = lane >> 5, j = job / SP, p = job % SP;
        *reinterpret_cast<u32x4*>(st.tile + n * 128 + (((2 * kq + hh) ^ (n & 7)) << 4)) = __builtin_bit_cast(u32x4, xin[4 * j + kq][p]);
    }
    static __device__ __forceinline__ void st_read(const Stash& st, Regs& r, int i, int lane) {
        const int row = 8 * i + (lane >> 3);
        r.sb[i] = *reinterpret_cast<const u32x4*>(st.tile + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
    }
    static __device__ __forceinline__ void st_store(const Stash& st, const Regs& r, int job, int i, int lane) {
        const int j = job / SP, p = job % SP;
        u32x4* dst = reinterpret_cast<u32x4*>(st.rows + p * st.plane + (long long)(8 * i + (lane >> 3)) * LD + j * 64 + (lane & 7) * 8);
        __builtin_nontemporal_store(r.sb[i], dst);
    }

    // ---- half 1 of position I: MFMAs on a0; fillers: read a1 (units H..U-1), then a job's global stores ----
    template <int I, int M>
    static __device__ __forceinline__ void h1_step(f32x16 (&acc)[NRBS], Regs& r, const bf16x8 (&xin)[KX][NS], const char* rd,
                                                   int lane, const Stash& st) {
        mfma_m<I, 0, M>(acc, r.a0, xin, r.bpe);
        constexpr int JS = job_st1(I);
        constexpr int NFILL = NF + (JS >= 0 ? 4 : 0);
#pragma unroll
        for (int k = 0; k < NFILL; ++k) {
            if ((k * NM) / NFILL == M) {
                if (k < NF) r.a1[k / NS][k % NS] = *reinterpret_cast<const bf16x8*>(rd + (H * NS + k) * 1024 + lane * 16);
                else if constexpr (JS >= 0) st_store(st, r, JS, k - NF, lane);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int I, int... M>
    static __device__ __forceinline__ void h1(f32x16 (&acc)[NRBS], Regs& r, const bf16x8 (&xin)[KX][NS], const char* rd, int lane,
                                              const Stash& st, std::integer_sequence<int, M...>) {
        (h1_step<I, M>(acc, r, xin, rd, lane, st), ...);
    }

    // ---- half 2: MFMAs on a1; fillers: D0 L0 D1 L1 ... (refill DMAs / next position's a0 reads), then a
    // stash job's 4 LDS writes and 4 read-backs (and its stores, when jobs come every position) ----
    static constexpr int dma_count(int i) { return (TRUNK ? SC::TRUNK_PIECES : SC::tail_pieces(T0 + i + SC::S)) / 4; }
    template <int I, int M>
    static __device__ __forceinline__ void h2_step(ChCtx& cx, f32x16 (&acc)[NRBS], Regs& r, const bf16x8 (&xin)[KX][NS],
                                                   const char* rd_next, unsigned dma_off, unsigned dma_dst, const Stash& st) {
        mfma_m<I, H, M>(acc, r.a1, xin, r.bpe);
        constexpr int ND = dma_count(I);
        constexpr int NL = (I + 1 < NPOS) ? NF : 0;
        constexpr int PAIRS = ND < NL ? ND : NL;
        constexpr int JW = job_wr(I), JS = job_st2(I);
        constexpr int NST = (JW >= 0 ? 8 : 0) + (JS >= 0 ? 4 : 0);
        constexpr int NFILL = ND + NL + NST;
#pragma unroll
        for (int k = 0; k < NFILL; ++k) {
            if ((k * NM) / (NFILL > 0 ? NFILL : 1) == M) {
                if (k < ND + NL) {
                    const bool is_dma = (k < 2 * PAIRS) ? (k % 2 == 0) : (ND > NL);
                    const int d = (k < 2 * PAIRS) ? k / 2 : k - PAIRS;
                    if (is_dma) {
                        // pieces go in pairs under one M0 save/restore (the odd one of a pair is a no-op filler)
                        if (d % 2 == 0) {
                            if (d + 1 < ND)
                                dma16s_x2(cx.gbase + dma_off, cx.voff[d], __builtin_amdgcn_readfirstlane(dma_dst + (unsigned)d * 4096u),
                                          cx.voff[d + 1], __builtin_amdgcn_readfirstlane(dma_dst + (unsigned)(d + 1) * 4096u));
                            else
                                dma16s(cx.gbase + dma_off, cx.voff[d], __builtin_amdgcn_readfirstlane(dma_dst + (unsigned)d * 4096u));
                        }
                    } else {
                        r.a0[d / NS][d % NS] = *reinterpret_cast<const bf16x8*>(rd_next + d * 1024 + cx.lane * 16);
                    }
                } else {
                    const int q = k - ND - NL;
                    if constexpr (JW >= 0) {
                        if (q < 4) st_write(st, xin, JW, q, cx.lane);
                        else if (q < 8) st_read(st, r, q - 4, cx.lane);
                    }
                    if constexpr (JS >= 0) {
                        if (q >= 8) st_store(st, r, JS, q - 8, cx.lane);
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    template <int I, int... M>
    static __device__ __forceinline__ void h2(ChCtx& cx, f32x16 (&acc)[NRBS], Regs& r, const bf16x8 (&xin)[KX][NS],
                                              const char* rd_next, unsigned dma_off, unsigned dma_dst, const Stash& st,
                                              std::integer_sequence<int, M...>) {
        (h2_step<I, M>(cx, acc, r, xin, rd_next, dma_off, dma_dst, st), ...);
    }

    template <int I>
    static __device__ __forceinline__ void pos(ChCtx& cx, f32x16 (&acc)[NRBS], const bf16x8 (&xin)[KX][NS], Regs& r,
                                               const char* peimg, int row, const Stash& st) {
        const int lane = cx.lane, hh = lane >> 5;
        if constexpr (BSRC != B_REG) {
#pragma unroll
            for (int kbl = 0; kbl < G; ++kbl)
#pragma unroll
                for (int p = 0; p < NS; ++p)
                    r.bpe[kbl][p] = *reinterpret_cast<const bf16x8*>(
                        peimg + p * PE_PLANE + swz(row, (BSRC == B_PED ? PE_X / 8 : 0) + 2 * (I * G + kbl) + hh, PE_ROW * 2));
        }
        __builtin_amdgcn_sched_barrier(0);
        h1<I>(acc, r, xin, cx.ring + cx.cslot * SC::SLOT, lane, st, std::make_integer_sequence<int, NM>{});
        // mid-step: my pieces of position +1 have landed; after the barrier everyone's have, and nobody
        // reads this position's slot any more (a1 is in registers: lgkmcnt(0) inside lds_barrier)
        wait_vm<(TRUNK ? SC::trunk_wait : SC::tail_wait(T0 + I)) + younger_stores(I)>();
        lds_barrier();
        const unsigned dma_dst = __builtin_amdgcn_readfirstlane(cx.ring_lds + (unsigned)cx.cslot * SC::SLOT + (unsigned)cx.w * 1024u);
        unsigned dma_off;
        if constexpr (TRUNK) {
            unsigned np = cx.trunk_pos + SC::S;
            if constexpr (SC::WRAP > 0) np = np >= (unsigned)SC::WRAP ? np - (unsigned)SC::WRAP : np;   // next tile restarts the stream
            dma_off = np * (unsigned)SC::SLOT;
            cx.trunk_pos += 1;
        } else {
            dma_off = SC::tail_off(T0 + I + SC::S);
        }

        cx.cslot = cx.cslot + 1 == SC::S ? 0 : cx.cslot + 1;
        __builtin_amdgcn_sched_barrier(0);
        h2<I>(cx, acc, r, xin, cx.ring + cx.cslot * SC::SLOT, dma_off, dma_dst, st, std::make_integer_sequence<int, NM>{});
    }

    template <int... I>
    static __device__ __forceinline__ void run_seq(ChCtx& cx, f32x16 (&acc)[NRBS], const bf16x8 (&xin)[KX][NS], const char* peimg,
                                                   int row, const Stash& st, std::integer_sequence<int, I...>) {
        Regs r;
        ch_loadA<NS, H>(r.a0, cx.ring + cx.cslot * SC::SLOT, 0, cx.lane);
        (pos<I>(cx, acc, xin, r, peimg, row, st), ...);
        // a job scheduled on the last position still owes its stores
        if constexpr (job_st1(NPOS) >= 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) st_store(st, r, job_st1(NPOS), i, cx.lane);
        }
    }
    static __device__ __forceinline__ void run(ChCtx& cx, f32x16 (&acc)[NRBS], const bf16x8 (&xin)[KX][NS], const char* peimg,
                                               int row, char* tile, __bf16* rows, long long plane) {
        Stash st{tile, rows, plane};
        run_seq(cx, acc, xin, peimg, row, st, std::make_integer_sequence<int, NPOS>{});
    }
};

template <class N, int NS, int DT, bool HAS_ALPHA, int NRBS, int G, int NPOS, int BSRC, bool TRUNK, int T0, int KX, int SP = 0, int LD = 1>
__device__ __forceinline__ void ch_phase(ChCtx& cx, f32x16 (&acc)[NRBS], const bf16x8 (&xin)[KX][NS], const char* peimg,
                                         int row, char* tile = nullptr, __bf16* rows = nullptr, long long plane = 0) {
    ChPhase<ChSched<N, NS, HAS_ALPHA>, NS, DT, NRBS, G, NPOS, BSRC, TRUNK, T0, KX, SP, LD>::run(cx, acc, xin, peimg, row, tile, rows, plane);
}

// acc[rb][q] = bias[32 rb + 16 (q>>3) + 8 h + (q&7)]  (the permuted row order), from the LDS copy
template <int NB>
__device__ __forceinline__ void ch_bias(f32x16 (&acc)[NB], const float* b, int h) {
#pragma unroll
    for (int rb = 0; rb < NB; ++rb) {
        const f32x4* p = reinterpret_cast<const f32x4*>(b + rb * 32 + 8 * h);
        const f32x4 v0 = p[0], v1 = p[1], v2 = p[4], v3 = p[5];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[rb][e] = v0[e];
            acc[rb][4 + e] = v1[e];
            acc[rb][8 + e] = v2[e];
            acc[rb][12 + e] = v3[e];
        }
    }
}

// Accumulators -> (ReLU) -> NS planes, in place as the next B operand: block rb gives k-blocks 2rb, 2rb+1.
// ReLU decisions (mask_index() records): bit q = "stored hi-plane value of accumulator q is non-zero",
// read off the packed 16-bit planes with v_pk_min_u16 (1 instruction per 2 values instead of a
// compare + select + or per value).  hi == 0 with acc > 0 needs acc below the smallest bf16 / half
// of the smallest fp16 subnormal: such a unit contributes nothing either way.
// REBIAS: as soon as row block rb is converted its accumulators are re-initialised with the biases of the NEXT phase
// (nextb, global memory), so those L2 loads have the rest of the conversion to land instead of stalling the first
// MFMAs of the next phase (bias loads issued at the phase start cost 9 % of the stash-writing forward).
template <int NS, int DT, bool RELU, int NB, int KX, bool MASK, bool REBIAS = false>
__device__ __forceinline__ void ch_convert(f32x16 (&acc)[NB], bf16x8 (&xin)[KX][NS], unsigned short* mrow, int lane,
                                           const float* __restrict__ nextb = nullptr) {
    static_assert(2 * NB <= KX, "activation planes do not fit");
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
#pragma unroll
    for (int rb = 0; rb < NB; ++rb) {
        unsigned word = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            u32x4 pk[NS];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v0 = acc[rb][8 * t + 2 * i], v1 = acc[rb][8 * t + 2 * i + 1];
                if (RELU && NS > 1) {   // on the bit patterns: max_i32(bits, 0) is +0 for every negative float and -0, identity otherwise
                                        // (a float max would add a canonicalising second v_max; inline asm draws hazard nops)
                    v0 = __builtin_bit_cast(float, max(__builtin_bit_cast(int, v0), 0));
                    v1 = __builtin_bit_cast(float, max(__builtin_bit_cast(int, v1), 0));
                }
                unsigned o[NS];
                split_pair<NS, DT>(v0, v1, o);
                if constexpr (RELU && NS == 1) {   // one plane: the same on the converted pair, one v_pk_max_i16 for two values
                    typedef __attribute__((ext_vector_type(2))) short s16x2;   // (rounding a negative value gives a negative value or -0)
                    const s16x2 z = {0, 0};
                    o[0] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, o[0]), z));
                }
#pragma unroll
                for (int p = 0; p < NS; ++p) pk[p][i] = o[p];
            }
#pragma unroll
            for (int p = 0; p < NS; ++p) xin[2 * rb + t][p] = __builtin_bit_cast(bf16x8, pk[p]);
            if constexpr (RELU && MASK) {
                const u32x4 hv = __builtin_bit_cast(u32x4, xin[2 * rb + t][0]);
                unsigned m = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned mi;   // 0/1 per halfword (as asm: LLVM rewrites umin(x, 1) into compare + select per halfword)
                    asm("v_pk_min_u16 %0, %1, %2" : "=v"(mi) : "v"(hv[i]), "s"(0x00010001u));
                    m |= mi << (2 * i);
                }
                word |= ((m | (m >> 15)) & 0xFFu) << (8 * t);       // values 2i (low halves) and 2i+1 (high halves)
            }
        }
        if constexpr (RELU && MASK) mrow[rb * 64] = (unsigned short)word;
        if constexpr (REBIAS) {
            const f32x4* p = reinterpret_cast<const f32x4*>(nextb + rb * 32 + 8 * (lane >> 5));
            const f32x4 v0 = p[0], v1 = p[1], v2 = p[4], v3 = p[5];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[rb][e] = v0[e];
                acc[rb][4 + e] = v1[e];
                acc[rb][8 + e] = v2[e];
                acc[rb][12 + e] = v3[e];
            }
        }
    }
}

// The first SP planes of KB k-blocks of xin to stash rows, outside any GEMM phase (4 k-blocks per pass through the wave's tile).
template <int NS, int SP, int KB, int KX, int LD>
__device__ __forceinline__ void ch_stash_all(const bf16x8 (&xin)[KX][NS], char* tile, __bf16* rows, long long plane, int lane) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    const int n = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int j = 0; j < KB / 4; ++j)
#pragma unroll
        for (int p = 0; p < SP; ++p) {
#pragma unroll
            for (int kq = 0; kq < 4; ++kq)
                *reinterpret_cast<u32x4*>(tile + n * 128 + (((2 * kq + hh) ^ (n & 7)) << 4)) = __builtin_bit_cast(u32x4, xin[4 * j + kq][p]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 8 * i + (lane >> 3);
                const u32x4 v = *reinterpret_cast<const u32x4*>(tile + row * 128 + (((lane & 7) ^ (row & 7)) << 4));
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(rows + p * plane + (long long)row * LD + j * 64 + (lane & 7) * 8));
            }
        }
}

template <class N, int NS, bool HAS_ALPHA, int DT, int SPK>
__global__ __launch_bounds__(CH_NT) void mlp_chain_fwd_kernel(const MlpFwdArgs A) {
    using SC = ChSched<N, NS, HAS_ALPHA>;
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, NRB = N::NRB, NRBV = N::NRBV, KKH = N::KKH;
    constexpr int PE_PLANE = CH_MT * PE_ROW * 2;
    constexpr int NBIAS = N::f32_w_rgb;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                  // [CH_S][SLOT]
    char* peimg = smem + CH_S * SC::SLOT;               // [NS][128 points][256 B], XOR-swizzled
    float* biasl = reinterpret_cast<float*>(peimg + NS * PE_PLANE);
    char* stage = reinterpret_cast<char*>(biasl + NBIAS);   // [4 waves][4 KiB] stash transposition tiles (SPK > 0)

    const int tid = threadIdx.x, lane = tid & 63;
    // (a live-point launch reads its point count on the device: include/lush_march.h "Live points")
    int P = A.P, n_tiles = A.n_tiles;
    if (A.live_cnt != nullptr) {
        P = __builtin_amdgcn_readfirstlane(*A.live_cnt);
        n_tiles = (P + 255) / 256 * 256 / CH_MT;      // (whole 256-point blocks, as the host pads a launch: the weight gradients read them)
    }
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    const char* wbase = reinterpret_cast<const char*>(A.wpk);
    {
        const float* f32 = reinterpret_cast<const float*>(wbase + (long long)N::total_entries * NS * 1024);
        for (int i = tid; i < NBIAS; i += CH_NT) biasl[i] = f32[i];
    }
    ChCtx cx;
    cx.ring = ring;
    cx.ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ring;
    cx.gbase = wbase + (long long)N::fwd2_base * NS * 1024;
    cx.cslot = 0;
    cx.trunk_pos = 0;
    cx.w = w;
    cx.lane = lane;
#pragma unroll
    for (int d = 0; d < 4; ++d) cx.voff[d] = (unsigned)lane * 16u + (unsigned)d * 4096u + (unsigned)w * 1024u;
#pragma unroll
    for (int j = 0; j < CH_S; ++j) ch_issue<SC::TRUNK_PIECES, SC::SLOT>(cx, (unsigned)j * SC::SLOT, j);

    constexpr bool stash_on = SPK > 0;
    constexpr int sp = SPK;
    const int row = w * 32 + n;
    char* tile_w = stage + w * 4096;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long pt0 = (long long)tile * CH_MT;
        const long long gpt = pt0 + row;
        const long long wpt = pt0 + w * 32;            // this wave's first point
        pe_tile<NS, CH_MT, CH_NT, DT>(peimg, PE_PLANE, PE_ROW * 2, A.rays, A.z, A.S, P, pt0, tid, A.live_idx);
        wait_vm<0>();      // first tile: the prologue DMAs; later tiles: already published by the last mid-step
        lds_barrier();
        if (stash_on) {
            for (int i = tid; i < sp * CH_MT * 12; i += CH_NT) {
                const int c = i % 12, pt = (i / 12) % CH_MT, p = i / (12 * CH_MT);
                const uint4 v = *reinterpret_cast<const uint4*>(peimg + p * PE_PLANE + swz(pt, c, PE_ROW * 2));
                *reinterpret_cast<uint4*>(A.pe + p * A.plane_pe + (pt0 + pt) * PE_ROW + c * 8) = v;
            }
        }
        cx.trunk_pos = 0;
        {   // opaque per tile: otherwise the ~40 static stream addresses of the tail are hoisted out of the
            // tile loop and live (spilled) across it
            unsigned long long gb = (unsigned long long)cx.gbase;
            asm volatile("" : "+s"(gb));
            cx.gbase = (const char*)gb;
        }
        // mask record of (this wave's 32-point block, layer ml, row block 0), this lane's 16-bit word
        const long long blk = pt0 / 32 + w;
        auto mrow = [&](int ml) -> unsigned short* {
            return stash_on ? reinterpret_cast<unsigned short*>(A.mask + ((blk * N::n_mask_layers + ml) * NRB) * 16) + lane : nullptr;
        };
        f32x16 acc[NRB];
        bf16x8 xin[KKH][NS];
        // ---- layer 0: gamma(x) from the PE image ----
        ch_bias<NRB>(acc, biasl + N::f32_b_trunk, h);
        ch_phase<N, NS, DT, HAS_ALPHA, NRB, SC::GT, N::KKX / SC::GT, B_PEX, true, 0, KKH>(cx, acc, xin, peimg, row);
        ch_convert<NS, DT, true, NRB, KKH, stash_on>(acc, xin, mrow(0), lane);
        // ---- layers 1 .. NL-1 ----
#pragma unroll 1
        for (int l = 1; l < NL; ++l) {
            ch_bias<NRB>(acc, biasl + N::f32_b_trunk + l * HW, h);
            if (l == N::SKIP)
                ch_phase<N, NS, DT, HAS_ALPHA, NRB, SC::GT, N::KKX / SC::GT, B_PEX, true, 0, KKH>(cx, acc, xin, peimg, row);
            ch_phase<N, NS, DT, HAS_ALPHA, NRB, SC::GT, KKH / SC::GT, B_REG, true, 0, KKH, SPK, HW>(cx, acc, xin, peimg, row, tile_w,
                                                                                 A.h0 + (l - 1) * A.h_stride + wpt * HW, A.plane_h);
            ch_convert<NS, DT, true, NRB, KKH, stash_on>(acc, xin, mrow(l), lane);
        }
        // ---- feature head (no activation) and alpha head, both on h_{NL-1} ----
        ch_bias<NRB>(acc, biasl + N::f32_b_feat, h);
        ch_phase<N, NS, DT, HAS_ALPHA, NRB, SC::GT, KKH / SC::GT, B_REG, false, 0, KKH, SPK, HW>(cx, acc, xin, peimg, row, tile_w,
                                                                              A.h0 + (NL - 1) * A.h_stride + wpt * HW, A.plane_h);
        float alpha = 0.f;
        if constexpr (HAS_ALPHA) {
            f32x16 aa[1];
            ch_bias<1>(aa, biasl + N::f32_b_alpha, h);
            ch_phase<N, NS, DT, HAS_ALPHA, 1, SC::G_A, SC::NP_A, B_REG, false, SC::T_A, KKH>(cx, aa, xin, peimg, row);
            alpha = aa[0][0];
        }
        ch_convert<NS, DT, false, NRB, KKH, false>(acc, xin, nullptr, lane);
        // ---- views layer: relu(Wv [feature ; gamma(d)] + b) ----
        f32x16 av[NRBV];
        ch_bias<NRBV>(av, biasl + N::f32_b_views, h);
        // (the feature activations are not stashed: FeatFactorArgs, lush_mlp.h)
        ch_phase<N, NS, DT, HAS_ALPHA, NRBV, SC::G_VA, SC::NP_VA, B_REG, false, SC::T_VA, KKH>(cx, av, xin, peimg, row);
        ch_phase<N, NS, DT, HAS_ALPHA, NRBV, SC::G_VB, SC::NP_VB, B_PED, false, SC::T_VB, KKH>(cx, av, xin, peimg, row);
        ch_convert<NS, DT, true, NRBV, KKH, stash_on>(av, xin, mrow(NL), lane);
        // ---- rgb head ----
        f32x16 ar[1];
        ch_bias<1>(ar, biasl + N::f32_b_rgb, h);
        if constexpr (SPK > 0) ch_stash_all<NS, SPK, N::KKV, KKH, HV>(xin, tile_w, A.hv + wpt * HV, A.plane_hv, lane);
        ch_phase<N, NS, DT, HAS_ALPHA, 1, SC::G_R, SC::NP_R, B_REG, false, SC::T_R, KKH>(cx, ar, xin, peimg, row);
        if (h == 0 && gpt < P && A.live_idx == nullptr) {      // (a live-point launch re-runs the forward for its stash only)
            float4 o;
            o.x = ar[0][0];
            o.y = ar[0][1];
            o.z = ar[0][2];
            o.w = HAS_ALPHA ? alpha : 0.f;
            *reinterpret_cast<float4*>(A.raw + gpt * 4) = o;
        }
    }
    wait_vm<0>();          // the look-ahead DMAs of the non-existent next tile must land before the LDS is released
}

// ----------------------------------------------------------------------------
// one-plane forward in 256 registers: TWO workgroups per CU
// ----------------------------------------------------------------------------
// The kernel above runs one wave per SIMD: whatever is not an MFMA (plane conversion, positional encoding, DMA issue,
// barrier waits) leaves the matrix pipe idle -- with one plane that is more than half of the time (per 128-point
// tile: 38 k cycles of MFMA in 81 k).  A second wave on the SIMD hides it only if the two are out of phase, and two
// waves of ONE workgroup never are (they meet at every position barrier; measured in round 1).  So the one-plane
// forward runs as two INDEPENDENT workgroups per CU -- own ring, own barriers, free to drift apart -- which needs the
// kernel in 256 registers and 80 KiB of LDS:
//   * every full-width layer is computed in two passes over K, rows 0..127 then rows 128..255 (NetT::fwd3 stream):
//     64 accumulators instead of 128; the first half is converted to its 8 k-blocks of the next B operand while the
//     second half runs, so the peak is 64 (acc) + 64 (B operand) + 32 (half of the next one);
//   * ring slots of 8 KiB (2 k-blocks x 4 row blocks), every segment cut into whole slots (uniform stream, WRAP per
//     tile, as in the backward kernel); biases come from L2 (their LDS copy does not fit 80 KiB).
template <class N>
struct HfSched {
    static constexpr int NS = 1, GT = 2, NRBH = N::NRB / 2;
#ifndef LUSH_HF_S
#define LUSH_HF_S 4
#endif
    static constexpr int S = LUSH_HF_S;                                    // ring slots
    static constexpr int TRUNK_PIECES = NRBH * NS * GT;                    // 8 pieces = 8 KiB per position
    static constexpr int SLOT = TRUNK_PIECES * 1024;
    static constexpr int trunk_wait = (S - 2) * TRUNK_PIECES / 4;
    static constexpr int G_A = TRUNK_PIECES, G_R = TRUNK_PIECES;            // 1-row-block segments: 8 k-blocks per position
    static constexpr int G_V = TRUNK_PIECES / N::NRBV;                     // views layer: NRBV row blocks
    static constexpr int NP_X = N::KKX / GT, NP_H = N::KKH / GT, NP_A = N::KKH / G_A, NP_VA = N::KKH / G_V,
                         NP_VB = N::KKD / G_V, NP_R = N::KKV / G_R;
    static constexpr int WRAP = 2 * NP_X + (N::NL - 1) * 2 * NP_H + (N::SKIP > 0 ? 2 * NP_X : 0) + 2 * NP_H + NP_A + NP_VA + NP_VB + NP_R;
    static_assert(N::NRB % 2 == 0 && N::NRBV == NRBH, "half-row kernel: the views layer is one half wide");
    static_assert(N::KKX % GT == 0 && N::KKH % GT == 0 && N::KKH % G_A == 0 && N::KKD % G_V == 0 && N::KKV % G_R == 0 &&
                  TRUNK_PIECES % 4 == 0, "segments must tile into whole positions");
    static_assert(N::fwd_END == WRAP * TRUNK_PIECES, "the half-row stream must cover the forward segments exactly");
    static constexpr int tail_pieces(int) { return TRUNK_PIECES; }     // (unused: every phase is TRUNK)
    static constexpr unsigned tail_off(int) { return 0; }
    static constexpr int tail_wait(int) { return trunk_wait; }
};

// acc[rb][q] = bias[32 rb + 16 (q>>3) + 8 h + (q&7)] straight from global memory (L2-resident fp32 block)
template <int NB>
__device__ __forceinline__ void ch_bias_g(f32x16 (&acc)[NB], const float* __restrict__ b, int h) {
#pragma unroll
    for (int rb = 0; rb < NB; ++rb) {
        const f32x4* p = reinterpret_cast<const f32x4*>(b + rb * 32 + 8 * h);
        const f32x4 v0 = p[0], v1 = p[1], v2 = p[4], v3 = p[5];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[rb][e] = v0[e];
            acc[rb][4 + e] = v1[e];
            acc[rb][8 + e] = v2[e];
            acc[rb][12 + e] = v3[e];
        }
    }
}

template <class N, int DT, int SPK>
__global__ __launch_bounds__(CH_NT, 2) void mlp_chain_fwd_half_kernel(const MlpFwdArgs A) {
    using SC = HfSched<N>;
    constexpr int NS = 1;
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, NRB = N::NRB, NRBH = N::NRB / 2, NRBV = N::NRBV, KKH = N::KKH;
    constexpr int PE_PLANE = CH_MT * PE_ROW * 2;
    static_assert(SPK <= 1, "one plane");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                  // [CH_S][SLOT]
    char* peimg = smem + SC::S * SC::SLOT;               // [128 points][256 B], XOR-swizzled
    char* stage = peimg + PE_PLANE;                     // [4 waves][4 KiB] stash transposition tiles

    const int tid = threadIdx.x, lane = tid & 63;
    // (a live-point launch reads its point count on the device: include/lush_march.h "Live points")
    int P = A.P, n_tiles = A.n_tiles;
    if (A.live_cnt != nullptr) {
        P = __builtin_amdgcn_readfirstlane(*A.live_cnt);
        n_tiles = (P + 255) / 256 * 256 / CH_MT;      // (whole 256-point blocks, as the host pads a launch: the weight gradients read them)
    }
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    const char* wbase = reinterpret_cast<const char*>(A.wpk);
    const float* f32b = reinterpret_cast<const float*>(wbase + (long long)N::total_entries * NS * 1024);
    ChCtx cx;
    cx.ring = ring;
    cx.ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ring;
    cx.gbase = wbase + (long long)N::fwd3_base * NS * 1024;
    cx.cslot = 0;
    cx.trunk_pos = 0;
    cx.w = w;
    cx.lane = lane;
#pragma unroll
    for (int d = 0; d < 4; ++d) cx.voff[d] = (unsigned)lane * 16u + (unsigned)d * 4096u + (unsigned)w * 1024u;
#pragma unroll
    for (int j = 0; j < SC::S; ++j) ch_issue<SC::TRUNK_PIECES, SC::SLOT>(cx, (unsigned)j * SC::SLOT, j);

    constexpr bool stash_on = SPK > 0;
    const int row = w * 32 + n;
    char* tile_w = stage + w * 4096;
    // Inference (no stash): the transposition tiles are free, so the fp32 bias block lives there and the per-layer
    // bias reads are LDS reads instead of 32 L2 loads per layer and lane (made visible by the first tile's barrier).
    static_assert(N::f32_w_rgb * 4 <= CH_NW * 4096, "the bias block must fit the stash tiles");
    if constexpr (SPK == 0) {
        for (int i = tid; i < N::f32_w_rgb; i += CH_NT) reinterpret_cast<float*>(stage)[i] = f32b[i];
    }
    const float* const bias = SPK == 0 ? reinterpret_cast<const float*>(stage) : f32b;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long pt0 = (long long)tile * CH_MT;
        const long long gpt = pt0 + row;
        const long long wpt = pt0 + w * 32;
        pe_tile<NS, CH_MT, CH_NT, DT>(peimg, PE_PLANE, PE_ROW * 2, A.rays, A.z, A.S, P, pt0, tid, A.live_idx);
        wait_vm<0>();      // first tile: the prologue DMAs; later tiles: already published by the last mid-step
        lds_barrier();
        if (SPK > 0) {
            for (int i = tid; i < CH_MT * 12; i += CH_NT) {
                const int c = i % 12, pt = i / 12;
                const uint4 v = *reinterpret_cast<const uint4*>(peimg + swz(pt, c, PE_ROW * 2));
                *reinterpret_cast<uint4*>(A.pe + (pt0 + pt) * PE_ROW + c * 8) = v;
            }
        }
        cx.trunk_pos = 0;
        {
            unsigned long long gb = (unsigned long long)cx.gbase;
            asm volatile("" : "+s"(gb));
            cx.gbase = (const char*)gb;
        }
        const long long blk = pt0 / 32 + w;
        auto mrow = [&](int ml, int half) -> unsigned short* {
            return stash_on ? reinterpret_cast<unsigned short*>(A.mask + ((blk * N::n_mask_layers + ml) * NRB + half * NRBH) * 16) + lane : nullptr;
        };
        f32x16 acc[NRBH];
        bf16x8 xin[KKH][NS], xnx[KKH][NS];
        typedef bf16x8 (&half_ref)[KKH / 2][NS];
        // ---- layer 0: gamma(x) from the PE image, two row halves ----
        // (with the stash on, every conversion re-initialises its accumulators with the next half-phase's biases:
        // the trunk and feature biases are contiguous, half-phase j = 2 l + half reads floats 128 j .. 128 j + 127)
        constexpr bool REB = SPK > 0;
        static_assert(N::f32_b_feat == N::f32_b_trunk + NL * HW, "feature biases follow the trunk biases");
        ch_bias_g<NRBH>(acc, bias + N::f32_b_trunk, h);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (!REB && half == 1) ch_bias_g<NRBH>(acc, bias + N::f32_b_trunk + (HW / 2), h);
            ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_X, B_PEX, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
            ch_convert<NS, DT, true, NRBH, KKH / 2, stash_on, REB>(acc, reinterpret_cast<half_ref>(xnx[half * (KKH / 2)]), mrow(0, half), lane,
                                                                   bias + N::f32_b_trunk + (half + 1) * (HW / 2));
        }
#pragma unroll
        for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        // ---- layers 1 .. NL-1 ----
#pragma unroll 1
        for (int l = 1; l < NL; ++l) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                if (!REB) ch_bias_g<NRBH>(acc, bias + N::f32_b_trunk + l * HW + half * (HW / 2), h);
                if (l == N::SKIP)
                    ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_X, B_PEX, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
                if (half == 0)      // the stash of h_{l-1} (this phase's B operand) rides in the first pass
                    ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, SPK, HW>::run(cx, acc, xin, peimg, row, tile_w,
                                                                                             A.h0 + (l - 1) * A.h_stride + wpt * HW, A.plane_h);
                else
                    ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
                ch_convert<NS, DT, true, NRBH, KKH / 2, stash_on, REB>(acc, reinterpret_cast<half_ref>(xnx[half * (KKH / 2)]), mrow(l, half), lane,
                                                                       bias + N::f32_b_trunk + (2 * l + half + 1) * (HW / 2));
            }
#pragma unroll
            for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        }
        // ---- feature head (no activation), two halves; then the alpha head, both on h_{NL-1} ----
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (!REB) ch_bias_g<NRBH>(acc, bias + N::f32_b_feat + half * (HW / 2), h);      // (REB: taken during the previous conversion)
            if (half == 0)
                ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, SPK, HW>::run(cx, acc, xin, peimg, row, tile_w,
                                                                                         A.h0 + (NL - 1) * A.h_stride + wpt * HW, A.plane_h);
            else
                ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
            // (the views biases are NOT taken early: the accumulators would stay live across the alpha phase and spill)
            if (half == 0)
                ch_convert<NS, DT, false, NRBH, KKH / 2, false, REB>(acc, reinterpret_cast<half_ref>(xnx[0]), nullptr, lane, bias + N::f32_b_feat + HW / 2);
            else
                ch_convert<NS, DT, false, NRBH, KKH / 2, false>(acc, reinterpret_cast<half_ref>(xnx[KKH / 2]), nullptr, lane);
        }
        float alpha;
        {
            f32x16 aa[1];
            ch_bias_g<1>(aa, bias + N::f32_b_alpha, h);
            ChPhase<SC, NS, DT, 1, SC::G_A, SC::NP_A, B_REG, true, 0, KKH, 0, 1>::run(cx, aa, xin, peimg, row, nullptr, nullptr, 0);
            alpha = aa[0][0];
        }
#pragma unroll
        for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        // ---- views layer: relu(Wv [feature ; gamma(d)] + b) ----
        ch_bias_g<NRBV>(acc, bias + N::f32_b_views, h);
        ChPhase<SC, NS, DT, NRBV, SC::G_V, SC::NP_VA, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
        ChPhase<SC, NS, DT, NRBV, SC::G_V, SC::NP_VB, B_PED, true, 0, KKH, 0, 1>::run(cx, acc, xin, peimg, row, nullptr, nullptr, 0);
        ch_convert<NS, DT, true, NRBV, KKH, stash_on>(acc, xin, mrow(NL, 0), lane);
        // ---- rgb head ----
        f32x16 ar[1];
        ch_bias_g<1>(ar, bias + N::f32_b_rgb, h);
        if constexpr (SPK > 0) ch_stash_all<NS, SPK, N::KKV, KKH, HV>(xin, tile_w, A.hv + wpt * HV, A.plane_hv, lane);
        ChPhase<SC, NS, DT, 1, SC::G_R, SC::NP_R, B_REG, true, 0, KKH, 0, 1>::run(cx, ar, xin, peimg, row, nullptr, nullptr, 0);
        if (h == 0 && gpt < P && A.live_idx == nullptr) {      // (a live-point launch re-runs the forward for its stash only)
            float4 o;
            o.x = ar[0][0];
            o.y = ar[0][1];
            o.z = ar[0][2];
            o.w = alpha;
            *reinterpret_cast<float4*>(A.raw + gpt * 4) = o;
        }
    }
    wait_vm<0>();          // the look-ahead DMAs of the non-existent next tile must land before the LDS is released
}

// ----------------------------------------------------------------------------
// backward chain: dZ_{l-1} = relu'(h_{l-1}) * (W_l^T dZ_l), down to d/d(point), d/d(viewdir)
// ----------------------------------------------------------------------------
// Same organisation as the forward (autograd of utils/run_lushnerf_helpers.py:394-423, 483-512): a wave
// keeps the gradient of its 32 points in registers from d_raw to d gamma; the transposed weights (bwd2
// copy, rows permuted by chain_row()) stream through the LDS ring.  Every segment is cut into positions
// of exactly NRB fragments (the 64-row d gamma(x) segments as 2 row blocks x NRB/2 k-blocks, the 32-row
// d gamma(d) segment as 1 x NRB), so the stream is uniform: position p at p * SLOT, WRAP positions per tile.
// Writes the dZ arrays the weight-gradient GEMMs read ([plane][point][cols] rows, through the same
// per-wave LDS transposition as the forward stash).
constexpr int BW_DPE_LD = 100;      // fp32 words per point in the d(gamma) scratch (96 used)

template <class N, int NS>
struct BwSched {
    static constexpr int GT = NS == 1 ? 2 : 1;                           // k-blocks per full-width position (see ChSched)
    static constexpr int S = CH_S;
    static constexpr int TRUNK_PIECES = N::NRB * NS * GT;
    static constexpr int SLOT = TRUNK_PIECES * 1024;
    static constexpr int trunk_wait = (CH_S - 2) * TRUNK_PIECES / 4;
    static constexpr int G_X = N::NRB * GT / 2, G_D = N::NRB * GT;       // k-blocks per position of the 2- and 1-row-block segments
    static constexpr int NP_VA = N::KKV / GT, NP_VB = N::KVB / G_D, NP_H = N::KKH / GT, NP_X = N::KKH / G_X;
    static constexpr int WRAP = NP_VA + NP_VB + NP_H * N::NL + (N::SKIP > 0 ? NP_X : 0) + NP_X;
    static_assert(N::KKV % GT == 0 && N::KVB % G_D == 0 && N::KKH % G_X == 0 && TRUNK_PIECES % 4 == 0, "backward stream positions must be uniform");
    static_assert((N::bwd_END - N::bwd_VAT) == WRAP * N::NRB * GT, "backward segments must tile into whole positions");
    static constexpr int tail_pieces(int) { return TRUNK_PIECES; }     // (unused: every phase is TRUNK)
    static constexpr unsigned tail_off(int) { return 0; }
    static constexpr int tail_wait(int) { return trunk_wait; }
};

// acc (* stored ReLU decision) -> NS planes, the next B operand
template <int NS, bool MASKED, int NB, int KX, int DT = DT_BF16>
__device__ __forceinline__ void bw_convert(const f32x16 (&acc)[NB], bf16x8 (&xin)[KX][NS], const unsigned (&mw)[NB]) {
    static_assert(2 * NB <= KX, "gradient planes do not fit");
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
#pragma unroll
    for (int rb = 0; rb < NB; ++rb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // stored decisions of the 8 values as 0/1 halfword pairs: X bit 2i = value 2i, bit 2i+16 = value 2i+1
            unsigned X = 0;
            if (MASKED) {
                const unsigned b = (mw[rb] >> (8 * t)) & 0xFFu;
                X = b | (b << 15);
            }
            u32x4 pk[NS];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned o[NS];
                split_pair<NS, DT>(acc[rb][8 * t + 2 * i], acc[rb][8 * t + 2 * i + 1], o);
#pragma unroll
                for (int p = 0; p < NS; ++p) {
                    if (MASKED) {   // x * {0,1} per halfword: zero where the ReLU was off (planes of a dropped value are both dropped)
                        const unsigned y = (X >> (2 * i)) & 0x00010001u;
                        asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(o[p]) : "v"(o[p]), "v"(y));
                    }
                    pk[p][i] = o[p];
                }
            }
#pragma unroll
            for (int p = 0; p < NS; ++p) xin[2 * rb + t][p] = __builtin_bit_cast(bf16x8, pk[p]);
        }
}

// The head gradients of this lane's point into the 8 extra columns of its dZv row (lanes 0..31): hi plane, lo plane.
template <int DT, int LDV, int HV>
__device__ __forceinline__ void bw_put_heads(__bf16* dzv, long long gpt, const float4& dr, int h) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    if (h == 0) {
        unsigned a[1], b[1], c[1], d[1];
        split_pair<1, DT>(dr.x, dr.y, a);
        split_pair<1, DT>(dr.z, dr.w, b);
        const float hx = elem_to_f32<DT>(__builtin_bit_cast(__bf16, (unsigned short)(a[0] & 0xFFFFu)));
        const float hy = elem_to_f32<DT>(__builtin_bit_cast(__bf16, (unsigned short)(a[0] >> 16)));
        const float hz = elem_to_f32<DT>(__builtin_bit_cast(__bf16, (unsigned short)(b[0] & 0xFFFFu)));
        const float hw = elem_to_f32<DT>(__builtin_bit_cast(__bf16, (unsigned short)(b[0] >> 16)));
        split_pair<1, DT>(dr.x - hx, dr.y - hy, c);
        split_pair<1, DT>(dr.z - hz, dr.w - hw, d);
        u32x4 v;
        v[0] = a[0]; v[1] = b[0]; v[2] = c[0]; v[3] = d[0];
        *reinterpret_cast<u32x4*>(dzv + gpt * LDV + HV) = v;
    }
}

template <int NB>
__device__ __forceinline__ void bw_zero(f32x16 (&acc)[NB]) {
#pragma unroll
    for (int rb = 0; rb < NB; ++rb)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[rb][q] = 0.f;
}

// all KB k-blocks x NS planes of xin to stash rows, outside any GEMM phase (4 k-blocks per pass through the wave's tile)
template <int NS, int KB, int KX, int LD>
__device__ __forceinline__ void bw_stash_all(const bf16x8 (&xin)[KX][NS], char* tile, __bf16* rows, long long plane, int lane) {
    ch_stash_all<NS, NS, KB, KX, LD>(xin, tile, rows, plane, lane);
}

// DT = DT_F16 (one plane): the gradient chain in fp16 with a per-launch power-of-two loss scale (A.scale[0], chosen from
// max|d_raw| by grad_scale_kernel so that scaled gradients sit far inside fp16's range): 11-bit operands at the cost
// of the 8-bit bf16 chain.  dZ rows are stored scaled; d(point) is un-scaled (A.scale[1]) on the way out and the
// weight-gradient GEMMs un-scale in their epilogue.
template <class N, int NS, bool HAS_ALPHA, int DT = DT_BF16>
__global__ __launch_bounds__(CH_NT) void mlp_chain_bwd_kernel(const MlpBwdArgs A) {
    using SC = BwSched<N, NS>;
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, NRB = N::NRB, NRBV = N::NRBV, KKH = N::KKH, KKV = N::KKV;
    constexpr int PARTS = CH_NT / CH_MT;
    static_assert(DT == DT_BF16 || NS == 1, "fp16 gradients are a single-plane format");
    float gscale = 1.f, ginv = 1.f;
    if constexpr (DT == DT_F16) { gscale = A.scale[0]; ginv = A.scale[1]; }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                              // [CH_S][SLOT]
    char* stage = smem + CH_S * SC::SLOT;                           // [4 waves][4 KiB]
    float* dpe = reinterpret_cast<float*>(stage + CH_NW * 4096);    // [128][BW_DPE_LD]
    float* dxbuf = dpe + CH_MT * BW_DPE_LD;                         // [PARTS][128][6]
    float* wtab = dxbuf + PARTS * CH_MT * 6;                        // w_rgb [3][HV] | w_alpha [HW]

    const int tid = threadIdx.x, lane = tid & 63;
    // (a live-point launch reads its point count on the device: include/lush_march.h "Live points")
    int P = A.P, n_tiles = A.n_tiles;
    if (A.live_cnt != nullptr) {
        P = __builtin_amdgcn_readfirstlane(*A.live_cnt);
        n_tiles = (P + 255) / 256 * 256 / CH_MT;      // (whole 256-point blocks, as the host pads a launch: the weight gradients read them)
    }
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    const char* wbase = reinterpret_cast<const char*>(A.wpk);
    {
        const float* f32 = reinterpret_cast<const float*>(wbase + (long long)N::total_entries * NS * 1024);
        for (int i = tid; i < 3 * HV + HW; i += CH_NT) wtab[i] = f32[N::f32_w_rgb + i];   // w_rgb then w_alpha are adjacent
    }
    static_assert(N::f32_w_alpha == N::f32_w_rgb + 3 * N::HV, "head matrices must be adjacent in the fp32 block");
    const float* w_rgb = wtab;
    const float* w_alpha = wtab + 3 * HV;
    ChCtx cx;
    cx.ring = ring;
    cx.ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ring;
    cx.gbase = wbase + (long long)N::bwd2_base * NS * 1024;
    cx.cslot = 0;
    cx.trunk_pos = 0;
    cx.w = w;
    cx.lane = lane;
#pragma unroll
    for (int d = 0; d < 4; ++d) cx.voff[d] = (unsigned)lane * 16u + (unsigned)d * 4096u + (unsigned)w * 1024u;
#pragma unroll
    for (int j = 0; j < CH_S; ++j) ch_issue<SC::TRUNK_PIECES, SC::SLOT>(cx, (unsigned)j * SC::SLOT, j);
    char* tile_w = stage + w * 4096;
    const int row = w * 32 + n;
    // VBT's K is zero-padded to KVB k-blocks: the planes it multiplies by 0 must hold finite values from the start
    bf16x8 xin[KKH][NS];
#pragma unroll
    for (int kb = 0; kb < KKH; ++kb)
#pragma unroll
        for (int p = 0; p < NS; ++p)
#pragma unroll
            for (int j = 0; j < 8; ++j) xin[kb][p][j] = (__bf16)0.f;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long pt0 = (long long)tile * CH_MT;
        const long long gpt = pt0 + row;
        const long long wpt = pt0 + w * 32;
        const long long blk = pt0 / 32 + w;
        cx.trunk_pos = 0;
        {
            unsigned long long gb = (unsigned long long)cx.gbase;
            asm volatile("" : "+s"(gb));
            cx.gbase = (const char*)gb;
        }
        auto mask_words = [&](unsigned (&mw)[NRB], int ml, int nb) {
            const unsigned short* m = reinterpret_cast<const unsigned short*>(A.mask + ((blk * N::n_mask_layers + ml) * NRB) * 16) + lane;
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) mw[rb] = rb < nb ? (unsigned)m[rb * 64] : 0u;
        };
        float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gpt < P) dr = *reinterpret_cast<const float4*>(A.draw + gpt * 4);
        if constexpr (DT == DT_F16) { dr.x *= gscale; dr.y *= gscale; dr.z *= gscale; dr.w *= gscale; }
        wait_vm<0>();          // first tile: the prologue DMAs (later tiles: published by the last mid-step)
        lds_barrier();         // also orders wtab and the previous tile's dpe/dxbuf traffic

        f32x16 acc[NRB];
        f32x16 apx[2], apd[1];
        bw_zero<2>(apx);
        bw_zero<1>(apd);
        unsigned mw[NRB];
        // ---- dZv = (Wrgb^T d_rgb) * relu'(hv)   (K = 3: rank-3 update on the VALU) ----
        mask_words(mw, NL, NRBV);
        {
            f32x16 av[NRBV];
#pragma unroll
            for (int rb = 0; rb < NRBV; ++rb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int f = 32 * rb + 16 * (q >> 3) + 8 * h + (q & 7);
                    av[rb][q] = w_rgb[f] * dr.x + w_rgb[HV + f] * dr.y + w_rgb[2 * HV + f] * dr.z;
                }
            unsigned mv[NRBV];
#pragma unroll
            for (int rb = 0; rb < NRBV; ++rb) mv[rb] = mw[rb];
            bw_convert<NS, true, NRBV, KKH, DT>(av, xin, mv);
        }
        // ---- d_feature = Wva^T dZv ; d gamma(d) = Wvb^T dZv ----
        bw_zero<NRB>(acc);
        constexpr int LDV = DzvLd<NS, HV>::v;
        if constexpr (NS == 1) bw_put_heads<DT, LDV, HV>(A.dzv, gpt, dr, h);
        ChPhase<SC, NS, DT, NRB, SC::GT, SC::NP_VA, B_REG, true, 0, KKH, NS, LDV>::run(cx, acc, xin, nullptr, row, tile_w, A.dzv + wpt * LDV, A.plane_hv);
        ChPhase<SC, NS, DT, 1, SC::G_D, SC::NP_VB, B_REG, true, 0, KKH, 0, 1>::run(cx, apd, xin, nullptr, row, nullptr, nullptr, 0);
        {
            unsigned none[NRB];
            bw_convert<NS, false, NRB, KKH, DT>(acc, xin, none);
        }
        // ---- dZ_{NL-1} = (Wfeat^T d_feature + Walpha^T d_alpha) * relu'(h_{NL-1}) ----
        mask_words(mw, NL - 1, NRB);
        bw_zero<NRB>(acc);
        // (d_feature is not stashed: FeatFactorArgs, lush_mlp.h)
        ChPhase<SC, NS, DT, NRB, SC::GT, SC::NP_H, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, nullptr, row, nullptr, nullptr, 0);
        if constexpr (HAS_ALPHA) {
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[rb][q] += w_alpha[32 * rb + 16 * (q >> 3) + 8 * h + (q & 7)] * dr.w;
        }
        bw_convert<NS, true, NRB, KKH, DT>(acc, xin, mw);
        // ---- trunk: dZ_{l-1} = (W_l^T dZ_l) * relu'(h_{l-1}) ----
#pragma unroll 1
        for (int l = NL - 1; l >= 1; --l) {
            mask_words(mw, l - 1, NRB);
            if (l == N::SKIP)     // gamma(x) rows of the skip layer's input
                ChPhase<SC, NS, DT, 2, SC::G_X, SC::NP_X, B_REG, true, 0, KKH, 0, 1>::run(cx, apx, xin, nullptr, row, nullptr, nullptr, 0);
            bw_zero<NRB>(acc);
            ChPhase<SC, NS, DT, NRB, SC::GT, SC::NP_H, B_REG, true, 0, KKH, NS, HW>::run(cx, acc, xin, nullptr, row, tile_w,
                                                                                      A.dz0 + l * A.dz_stride + wpt * HW, A.plane_h);
            bw_convert<NS, true, NRB, KKH, DT>(acc, xin, mw);
            asm volatile("" ::"v"(xin[0][0]), "v"(xin[KKH - 1][0]));
        }
        // ---- layer 0: d gamma(x) += W_0^T dZ_0 ----
        ChPhase<SC, NS, DT, 2, SC::G_X, SC::NP_X, B_REG, true, 0, KKH, 0, 1>::run(cx, apx, xin, nullptr, row, nullptr, nullptr, 0);
        bw_stash_all<NS, KKH, KKH, HW>(xin, tile_w, A.dz0 + wpt * HW, A.plane_h, lane);
        // ---- through the encoding: d/dx_i = g[i] + sum_k 2^k (cos(2^k x_i) g_sin - sin(2^k x_i) g_cos) ----
        {
            float* g = dpe + row * BW_DPE_LD + 8 * h;       // this lane's columns: 32b + 16t + 8h + (0..7)
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x16& a = b < 2 ? apx[b] : apd[0];
                    f32x4 v0 = {a[8 * t], a[8 * t + 1], a[8 * t + 2], a[8 * t + 3]};
                    f32x4 v1 = {a[8 * t + 4], a[8 * t + 5], a[8 * t + 6], a[8 * t + 7]};
                    *reinterpret_cast<f32x4*>(g + 32 * b + 16 * t) = v0;
                    *reinterpret_cast<f32x4*>(g + 32 * b + 16 * t + 4) = v1;
                }
        }
        lds_barrier();
        {
            const int pt = tid % CH_MT, part = tid / CH_MT;
            const long long gp = pt0 + pt;
            float x[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
            if (gp < P) point_of(A.rays, A.z, A.S, A.live_idx ? (long long)A.live_idx[gp] : gp, x, d);
            float gx[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
            const float* g = dpe + pt * BW_DPE_LD;
            for (int u = part; u < L_X + L_D; u += PARTS) {
                const bool isd = u >= L_X;
                const int k = isd ? u - L_X : u;
                const int base = isd ? PE_X : 0;
                const float f = (float)(1 << k);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float v = isd ? d[i] : x[i];
                    float sn, cs;
                    lush_sincos(v * f, &sn, &cs);
                    float t = f * (cs * g[base + 3 + 6 * k + i] - sn * g[base + 3 + 6 * k + 3 + i]);
                    if (k == 0) t += g[base + i];
                    if (isd) gd[i] += t; else gx[i] += t;
                }
            }
            float* o = dxbuf + (part * CH_MT + pt) * 6;
            o[0] = gx[0]; o[1] = gx[1]; o[2] = gx[2]; o[3] = gd[0]; o[4] = gd[1]; o[5] = gd[2];
        }
        lds_barrier();
        for (int i = tid; i < CH_MT * 6; i += CH_NT) {
            const int pt = i / 6, c = i % 6;
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < PARTS; ++p) sum += dxbuf[(p * CH_MT + pt) * 6 + c];
            const long long gp = pt0 + pt;
            if (gp < P) {
                A.dpts[gp * 8 + (c < 3 ? c : c + 1)] = sum * ginv;
                if (c % 3 == 2) A.dpts[gp * 8 + (c < 3 ? 3 : 7)] = 0.f;      // the pad columns are zeros, as the wide kernels write them (include/lush_march.h)
            }
        }
    }
    wait_vm<0>();
}

// ----------------------------------------------------------------------------
// one-plane backward chain in 256 registers: TWO workgroups per CU (see mlp_chain_fwd_half_kernel)
// ----------------------------------------------------------------------------
// Same half-row scheme on the transposed weights (NetT::bwd3 stream): 64 accumulators, the first half of dZ_{l-1} is
// masked and converted while the second half runs.  LDS per workgroup <= 80 KiB: ring 4 x 8 KiB, the per-wave stash
// tiles (also the scratch of the final reduction), the d(gamma) image in the chain's 16-bit type (fp32 would be
// 51 KiB; used for the loss-scaled fp16 chain only, where 11 bits match the chain's own operands), the two K<=3 head matrices.  The d(gamma) partial sums are parked in that image between their phases
// (one extra 16-bit rounding of the skip layer's share) because the accumulators are needed for the trunk.
constexpr int BH_DPE_LD = 104;      // 16-bit elements per point in the d(gamma) image (96 used; rows stay 16-byte aligned)

template <class N>
struct HbSched {
    static constexpr int NS = 1, GT = 2, NRBH = N::NRB / 2;
    static constexpr int S = 4;
    static constexpr int TRUNK_PIECES = NRBH * NS * GT;                    // 8 KiB per position
    static constexpr int SLOT = TRUNK_PIECES * 1024;
    static constexpr int trunk_wait = (S - 2) * TRUNK_PIECES / 4;
    static constexpr int G_X = TRUNK_PIECES / 2, G_D = TRUNK_PIECES;       // k-blocks per position of the 2- and 1-row-block segments
    static constexpr int NP_VA = N::KKV / GT, NP_VB = N::KVB / G_D, NP_H = N::KKH / GT, NP_X = N::KKH / G_X;
    static constexpr int WRAP = 2 * NP_VA + NP_VB + 2 * NP_H * N::NL + (N::SKIP > 0 ? NP_X : 0) + NP_X;
    static_assert(N::KKV % GT == 0 && N::KVB % G_D == 0 && N::KKH % G_X == 0 && N::KKH % GT == 0, "backward stream positions must be uniform");
    static_assert((N::bwd_END - N::bwd_VAT) == WRAP * TRUNK_PIECES, "backward segments must tile into whole positions");
    static constexpr int tail_pieces(int) { return TRUNK_PIECES; }
    static constexpr unsigned tail_off(int) { return 0; }
    static constexpr int tail_wait(int) { return trunk_wait; }
};

template <class N, bool HAS_ALPHA, int DT>
__global__ __launch_bounds__(CH_NT, 2) void mlp_chain_bwd_half_kernel(const MlpBwdArgs A) {
    using SC = HbSched<N>;
    constexpr int NS = 1;
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, NRB = N::NRB, NRBH = N::NRB / 2, NRBV = N::NRBV, KKH = N::KKH;
    constexpr int PARTS = CH_NT / CH_MT;
    static_assert(NRBV == NRBH, "the views layer is one half wide");
    float gscale = 1.f, ginv = 1.f;
    if constexpr (DT == DT_F16) { gscale = A.scale[0]; ginv = A.scale[1]; }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* ring = smem;                                              // [S][SLOT]
    char* stage = smem + SC::S * SC::SLOT;                          // [4 waves][4 KiB]; reused as dxbuf [PARTS][128][6] fp32
    __bf16* dpe = reinterpret_cast<__bf16*>(stage + CH_NW * 4096);  // [128][BH_DPE_LD] in the chain's 16-bit type
    float* wtab = reinterpret_cast<float*>(dpe + CH_MT * BH_DPE_LD);   // w_rgb [3][HV] | w_alpha [HW]
    float* dxbuf = reinterpret_cast<float*>(stage);
    static_assert(PARTS * CH_MT * 6 * 4 <= CH_NW * 4096, "the reduction scratch must fit the stash tiles");

    const int tid = threadIdx.x, lane = tid & 63;
    // (a live-point launch reads its point count on the device: include/lush_march.h "Live points")
    int P = A.P, n_tiles = A.n_tiles;
    if (A.live_cnt != nullptr) {
        P = __builtin_amdgcn_readfirstlane(*A.live_cnt);
        n_tiles = (P + 255) / 256 * 256 / CH_MT;      // (whole 256-point blocks, as the host pads a launch: the weight gradients read them)
    }
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    const char* wbase = reinterpret_cast<const char*>(A.wpk);
    {
        const float* f32 = reinterpret_cast<const float*>(wbase + (long long)N::total_entries * NS * 1024);
        for (int i = tid; i < 3 * HV + HW; i += CH_NT) wtab[i] = f32[N::f32_w_rgb + i];
    }
    const float* w_rgb = wtab;
    const float* w_alpha = wtab + 3 * HV;
    ChCtx cx;
    cx.ring = ring;
    cx.ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ring;
    cx.gbase = wbase + (long long)N::bwd3_base * NS * 1024;
    cx.cslot = 0;
    cx.trunk_pos = 0;
    cx.w = w;
    cx.lane = lane;
#pragma unroll
    for (int d = 0; d < 4; ++d) cx.voff[d] = (unsigned)lane * 16u + (unsigned)d * 4096u + (unsigned)w * 1024u;
#pragma unroll
    for (int j = 0; j < SC::S; ++j) ch_issue<SC::TRUNK_PIECES, SC::SLOT>(cx, (unsigned)j * SC::SLOT, j);
    char* tile_w = stage + w * 4096;
    const int row = w * 32 + n;
    bf16x8 xin[KKH][NS], xnx[KKH][NS];
    typedef bf16x8 (&half_ref)[KKH / 2][NS];
#pragma unroll
    for (int kb = 0; kb < KKH; ++kb)
#pragma unroll
        for (int j = 0; j < 8; ++j) { xin[kb][0][j] = (__bf16)0.f; xnx[kb][0][j] = (__bf16)0.f; }

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long pt0 = (long long)tile * CH_MT;
        const long long gpt = pt0 + row;
        const long long wpt = pt0 + w * 32;
        const long long blk = pt0 / 32 + w;
        cx.trunk_pos = 0;
        {
            unsigned long long gb = (unsigned long long)cx.gbase;
            asm volatile("" : "+s"(gb));
            cx.gbase = (const char*)gb;
        }
        // ReLU decisions of (layer ml, row half): this lane's 16-bit words of the 4 row blocks
        auto mask_words = [&](unsigned (&mw)[NRBH], int ml, int half) {
            const unsigned short* m = reinterpret_cast<const unsigned short*>(A.mask + ((blk * N::n_mask_layers + ml) * NRB + half * NRBH) * 16) + lane;
#pragma unroll
            for (int rb = 0; rb < NRBH; ++rb) mw[rb] = (unsigned)m[rb * 64];
        };
        float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gpt < P) dr = *reinterpret_cast<const float4*>(A.draw + gpt * 4);
        if constexpr (DT == DT_F16) { dr.x *= gscale; dr.y *= gscale; dr.z *= gscale; dr.w *= gscale; }
        wait_vm<0>();
        lds_barrier();         // also orders wtab and the previous tile's dpe / dxbuf traffic

        f32x16 acc[NRBH];
        unsigned mw[NRBH];
        // d(gamma) columns 32b..32b+31 of this lane's point, 16-bit: rows are wave-private until the barrier below
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
        __bf16* const grow = dpe + row * BH_DPE_LD + 8 * h;       // this lane's columns: 32b + 16t + 8h + (0..7)
        auto dpe_put = [&](const f32x16& a, int b) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                u32x4 pk;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned o[1];
                    split_pair<1, DT>(a[8 * t + 2 * i], a[8 * t + 2 * i + 1], o);
                    pk[i] = o[0];
                }
                *reinterpret_cast<u32x4*>(grow + 32 * b + 16 * t) = pk;
            }
        };
        auto dpe_add = [&](f32x16& a, int b) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(grow + 32 * b + 16 * t);
#pragma unroll
                for (int i = 0; i < 8; ++i) a[8 * t + i] += elem_to_f32<DT>(v[i]);
            }
        };
        // ---- dZv = (Wrgb^T d_rgb) * relu'(hv)   (K = 3: rank-3 update on the VALU) ----
        mask_words(mw, NL, 0);
#pragma unroll
        for (int rb = 0; rb < NRBV; ++rb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int f = 32 * rb + 16 * (q >> 3) + 8 * h + (q & 7);
                acc[rb][q] = w_rgb[f] * dr.x + w_rgb[HV + f] * dr.y + w_rgb[2 * HV + f] * dr.z;
            }
        bw_convert<NS, true, NRBV, KKH, DT>(acc, xin, mw);
        // ---- d_feature = Wva^T dZv (two row halves); d gamma(d) = Wvb^T dZv ----
        constexpr int LDV = DzvLd<NS, HV>::v;
        bw_put_heads<DT, LDV, HV>(A.dzv, gpt, dr, h);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            bw_zero<NRBH>(acc);
            if (half == 0)
                ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_VA, B_REG, true, 0, KKH, NS, LDV>::run(cx, acc, xin, nullptr, row, tile_w, A.dzv + wpt * LDV, A.plane_hv);
            else
                ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_VA, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, nullptr, row, nullptr, nullptr, 0);
            unsigned none[NRBH];
            bw_convert<NS, false, NRBH, KKH / 2, DT>(acc, reinterpret_cast<half_ref>(xnx[half * (KKH / 2)]), none);
        }
        {
            f32x16 apd[1];
            bw_zero<1>(apd);
            ChPhase<SC, NS, DT, 1, SC::G_D, SC::NP_VB, B_REG, true, 0, KKH, 0, 1>::run(cx, apd, xin, nullptr, row, nullptr, nullptr, 0);
            dpe_put(apd[0], 2);
        }
#pragma unroll
        for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        // ---- dZ_{NL-1} = (Wfeat^T d_feature + Walpha^T d_alpha) * relu'(h_{NL-1}) ----
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            mask_words(mw, NL - 1, half);
            bw_zero<NRBH>(acc);
            ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, nullptr, row, nullptr, nullptr, 0);
            if constexpr (HAS_ALPHA) {
#pragma unroll
                for (int rb = 0; rb < NRBH; ++rb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[rb][q] += w_alpha[half * (HW / 2) + 32 * rb + 16 * (q >> 3) + 8 * h + (q & 7)] * dr.w;
            }
            bw_convert<NS, true, NRBH, KKH / 2, DT>(acc, reinterpret_cast<half_ref>(xnx[half * (KKH / 2)]), mw);
        }
#pragma unroll
        for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        // ---- trunk: dZ_{l-1} = (W_l^T dZ_l) * relu'(h_{l-1}) ----
#pragma unroll 1
        for (int l = NL - 1; l >= 1; --l) {
            if (l == N::SKIP) {   // gamma(x) rows of the skip layer's input, parked in the image until layer 0 adds its share
                f32x16 apx[2];
                bw_zero<2>(apx);
                ChPhase<SC, NS, DT, 2, SC::G_X, SC::NP_X, B_REG, true, 0, KKH, 0, 1>::run(cx, apx, xin, nullptr, row, nullptr, nullptr, 0);
                dpe_put(apx[0], 0);
                dpe_put(apx[1], 1);
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                mask_words(mw, l - 1, half);
                bw_zero<NRBH>(acc);
                if (half == 0)
                    ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, NS, HW>::run(cx, acc, xin, nullptr, row, tile_w,
                                                                                              A.dz0 + l * A.dz_stride + wpt * HW, A.plane_h);
                else
                    ChPhase<SC, NS, DT, NRBH, SC::GT, SC::NP_H, B_REG, true, 0, KKH, 0, 1>::run(cx, acc, xin, nullptr, row, nullptr, nullptr, 0);
                bw_convert<NS, true, NRBH, KKH / 2, DT>(acc, reinterpret_cast<half_ref>(xnx[half * (KKH / 2)]), mw);
            }
#pragma unroll
            for (int k = 0; k < KKH; ++k) xin[k][0] = xnx[k][0];
        }
        // ---- layer 0: d gamma(x) += W_0^T dZ_0 ----
        {
            f32x16 apx[2];
            bw_zero<2>(apx);
            ChPhase<SC, NS, DT, 2, SC::G_X, SC::NP_X, B_REG, true, 0, KKH, 0, 1>::run(cx, apx, xin, nullptr, row, nullptr, nullptr, 0);
            bw_stash_all<NS, KKH, KKH, HW>(xin, tile_w, A.dz0 + wpt * HW, A.plane_h, lane);
            if constexpr (N::SKIP > 0) { dpe_add(apx[0], 0); dpe_add(apx[1], 1); }
            dpe_put(apx[0], 0);
            dpe_put(apx[1], 1);
        }
        // ---- through the encoding: d/dx_i = g[i] + sum_k 2^k (cos(2^k x_i) g_sin - sin(2^k x_i) g_cos) ----
        lds_barrier();         // d(gamma) image complete; every wave has left its stash tile (dxbuf aliases them)
        {
            const int pt = tid % CH_MT, part = tid / CH_MT;
            const long long gp = pt0 + pt;
            float x[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
            if (gp < P) point_of(A.rays, A.z, A.S, A.live_idx ? (long long)A.live_idx[gp] : gp, x, d);
            float gx[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f};
            const __bf16* g = dpe + pt * BH_DPE_LD;
            auto gv = [&](int c) { return elem_to_f32<DT>(g[c]); };
            for (int u = part; u < L_X + L_D; u += PARTS) {
                const bool isd = u >= L_X;
                const int k = isd ? u - L_X : u;
                const int base = isd ? PE_X : 0;
                const float f = (float)(1 << k);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float v = isd ? d[i] : x[i];
                    float sn, cs;
                    lush_sincos(v * f, &sn, &cs);
                    float t = f * (cs * gv(base + 3 + 6 * k + i) - sn * gv(base + 3 + 6 * k + 3 + i));
                    if (k == 0) t += gv(base + i);
                    if (isd) gd[i] += t; else gx[i] += t;
                }
            }
            float* o = dxbuf + (part * CH_MT + pt) * 6;
            o[0] = gx[0]; o[1] = gx[1]; o[2] = gx[2]; o[3] = gd[0]; o[4] = gd[1]; o[5] = gd[2];
        }
        lds_barrier();
        for (int i = tid; i < CH_MT * 6; i += CH_NT) {
            const int pt = i / 6, c = i % 6;
            float sum = 0.f;
#pragma unroll
            for (int p = 0; p < PARTS; ++p) sum += dxbuf[(p * CH_MT + pt) * 6 + c];
            const long long gp = pt0 + pt;
            if (gp < P) {
                A.dpts[gp * 8 + (c < 3 ? c : c + 1)] = sum * ginv;
                if (c % 3 == 2) A.dpts[gp * 8 + (c < 3 ? 3 : 7)] = 0.f;      // the pad columns are zeros, as the wide kernels write them (include/lush_march.h)
            }
        }
    }
    wait_vm<0>();
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
template <class N, int NS, bool HAS_ALPHA>
static size_t chain_lds_bytes() {
    return (size_t)CH_S * ChSched<N, NS, HAS_ALPHA>::SLOT + (size_t)NS * CH_MT * PE_ROW * 2 + (size_t)N::f32_w_rgb * 4 +
           (size_t)CH_NW * 4096;
}

template <class N, int NS, bool HAS_ALPHA, int DT, int SPK>
static int launch_chain_sp(const MlpFwdArgs& a, hipStream_t s) {
    auto k = mlp_chain_fwd_kernel<N, NS, HAS_ALPHA, DT, SPK>;
    const size_t lds = chain_lds_bytes<N, NS, HAS_ALPHA>();
    static KernelOnce once;
    int dev = 0, n_cu = 0;
    if (int rc = current_device_cus(dev, n_cu)) return rc;
    if (int rc = kernel_lds_once(once, dev, reinterpret_cast<const void*>(k), lds)) return rc;
    const int grid = a.n_tiles < n_cu ? a.n_tiles : n_cu;     // one workgroup per CU, tiles strided
    hipLaunchKernelGGL(k, dim3(grid), dim3(CH_NT), lds, s, a);
    LUSH_HIP(hipGetLastError());
    return 0;
}

template <class N, int DT, int SPK>
static int launch_chain_half_sp(const MlpFwdArgs& a, hipStream_t s) {
    auto k = mlp_chain_fwd_half_kernel<N, DT, SPK>;
    const size_t lds = (size_t)HfSched<N>::S * HfSched<N>::SLOT + (size_t)CH_MT * PE_ROW * 2 + (size_t)CH_NW * 4096;
    static KernelOnce once;
    int dev = 0, n_cu = 0;
    if (int rc = current_device_cus(dev, n_cu)) return rc;
    if (int rc = kernel_lds_once(once, dev, reinterpret_cast<const void*>(k), lds)) return rc;
    const int grid = a.n_tiles < 2 * n_cu ? a.n_tiles : 2 * n_cu;     // two workgroups per CU, tiles strided
    hipLaunchKernelGGL(k, dim3(grid), dim3(CH_NT), lds, s, a);
    LUSH_HIP(hipGetLastError());
    return 0;
}

template <class N, int NS, bool HAS_ALPHA, int DT>
static int launch_chain_k(const MlpFwdArgs& a, int variant, hipStream_t s) {
    const int sp = a.write_stash ? a.stash_planes : 0;
    if constexpr (NS == 1 && HAS_ALPHA && N::HW == 256) {
        if constexpr (DT == DT_F16) {      // the headline forward: 64 points per wave unless a variant bit selects an older kernel
            if (!(variant & (LUSH_VARIANT_FWD_HALF | LUSH_VARIANT_FWD_512)) && sp <= 1) return launch_mlp_wide_fwd(a, s);
        }
        if (!(variant & LUSH_VARIANT_FWD_512)) {
            if (sp == 0) return launch_chain_half_sp<N, DT, 0>(a, s);
            if (sp == 1) return launch_chain_half_sp<N, DT, 1>(a, s);
        }
    }
    if (sp == 0) return launch_chain_sp<N, NS, HAS_ALPHA, DT, 0>(a, s);
    if (sp == 1) return launch_chain_sp<N, NS, HAS_ALPHA, DT, 1>(a, s);
    if constexpr (NS == 2) {
        if (sp == 2) return launch_chain_sp<N, NS, HAS_ALPHA, DT, 2>(a, s);
    }
    return set_error("launch_mlp_chain_fwd: bad stash plane count");
}

// planes 1, 2 and the fp16 code run on the chain kernel (128-point tiles); 3 planes keep mlp_fwd_kernel.
bool mlp_fwd_chain_enabled(int planes) { return planes == 1 || planes == 2 || planes == PLANES_F16; }

int launch_mlp_chain_fwd(int net, int planes, const MlpFwdArgs& a, int variant, hipStream_t s) {
    if (planes == PLANES_F16) {
        if (net == 0) return launch_chain_k<NetNerf, 1, true, DT_F16>(a, variant, s);
        return launch_chain_k<NetNoise, 1, false, DT_F16>(a, variant, s);
    }
    if (net == 0) {
        if (planes == 1) return launch_chain_k<NetNerf, 1, true, DT_BF16>(a, variant, s);
        if (planes == 2) return launch_chain_k<NetNerf, 2, true, DT_BF16>(a, variant, s);
    } else {
        if (planes == 1) return launch_chain_k<NetNoise, 1, false, DT_BF16>(a, variant, s);
        if (planes == 2) return launch_chain_k<NetNoise, 2, false, DT_BF16>(a, variant, s);
    }
    return set_error("launch_mlp_chain_fwd: bad net/planes");
}

template <class N, int NS, bool HAS_ALPHA, int DT = DT_BF16>
static int launch_chain_bwd_k(const MlpBwdArgs& a, hipStream_t s) {
    auto k = mlp_chain_bwd_kernel<N, NS, HAS_ALPHA, DT>;
    const size_t lds = (size_t)CH_S * BwSched<N, NS>::SLOT + (size_t)CH_NW * 4096 + (size_t)CH_MT * BW_DPE_LD * 4 +
                       (size_t)(CH_NT / CH_MT) * CH_MT * 6 * 4 + (size_t)(3 * N::HV + N::HW) * 4;
    static KernelOnce once;
    int dev = 0, n_cu = 0;
    if (int rc = current_device_cus(dev, n_cu)) return rc;
    if (int rc = kernel_lds_once(once, dev, reinterpret_cast<const void*>(k), lds)) return rc;
    const int grid = a.n_tiles < n_cu ? a.n_tiles : n_cu;
    hipLaunchKernelGGL(k, dim3(grid), dim3(CH_NT), lds, s, a);
    LUSH_HIP(hipGetLastError());
    return 0;
}

// 1 and 2 planes run on the chain kernel (128-point tiles); 3 planes keep mlp_bwd_kernel.
bool mlp_bwd_chain_enabled(int planes) { return planes == 1 || planes == 2 || planes == PLANES_F16; }

template <class N, bool HAS_ALPHA, int DT>
static int launch_chain_bwd_half(const MlpBwdArgs& a, hipStream_t s) {
    auto k = mlp_chain_bwd_half_kernel<N, HAS_ALPHA, DT>;
    const size_t lds = (size_t)HbSched<N>::S * HbSched<N>::SLOT + (size_t)CH_NW * 4096 + (size_t)CH_MT * BH_DPE_LD * 2 +
                       (size_t)(3 * N::HV + N::HW) * 4;
    static KernelOnce once;
    int dev = 0, n_cu = 0;
    if (int rc = current_device_cus(dev, n_cu)) return rc;
    if (int rc = kernel_lds_once(once, dev, reinterpret_cast<const void*>(k), lds)) return rc;
    const int grid = a.n_tiles < 2 * n_cu ? a.n_tiles : 2 * n_cu;     // two workgroups per CU
    hipLaunchKernelGGL(k, dim3(grid), dim3(CH_NT), lds, s, a);
    LUSH_HIP(hipGetLastError());
    return 0;
}

int launch_mlp_chain_bwd(int net, int planes, const MlpBwdArgs& a, int variant, hipStream_t s) {
    if (planes == PLANES_F16) {
        if (a.scale == nullptr) return set_error("launch_mlp_chain_bwd: the fp16 chain needs its loss scale");
        if (net == 0) {     // the headline backward: 64 points per wave unless a variant bit selects an older kernel
            if (variant & LUSH_VARIANT_BWD_512) return launch_chain_bwd_k<NetNerf, 1, true, DT_F16>(a, s);
            if (variant & LUSH_VARIANT_BWD_HALF) return launch_chain_bwd_half<NetNerf, true, DT_F16>(a, s);
            return launch_mlp_wide_bwd(a, s);
        }
        return launch_chain_bwd_k<NetNoise, 1, false, DT_F16>(a, s);
    }
    if (net == 0) {
        // (plain bf16 keeps the one-workgroup kernel: its d(gamma) image is fp32, the half-row kernel's is 16-bit, and
        // 8 mantissa bits there moved the 40-step training trajectory of the (h,1) mode from 6e-4 to 1.2e-3..2.2e-3)
        if (planes == 1) return launch_chain_bwd_k<NetNerf, 1, true>(a, s);
        if (planes == 2) return launch_chain_bwd_k<NetNerf, 2, true>(a, s);
    } else {
        if (planes == 1) return launch_chain_bwd_k<NetNoise, 1, false>(a, s);
        if (planes == 2) return launch_chain_bwd_k<NetNoise, 2, false>(a, s);
    }
    return set_error("launch_mlp_chain_bwd: bad net/planes");
}

}  // namespace lush
