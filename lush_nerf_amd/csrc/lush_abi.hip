// lush-march: C ABI of the fused MLP path (pack plan, stash layout, launch order).
#include "lush_common.h"
#include "lush_host.h"
#include <cstring>
#include <vector>
#include "../../include/lush_march.h"
#include "../../include/lush_live_fwd.h"

using namespace lush;

namespace {

struct NetInfo { int HW, NL, SKIP, HV, NRB, total_entries, f32_total; };
template <class N> NetInfo info_of() { return {N::HW, N::NL, N::SKIP, N::HV, N::NRB, N::total_entries, N::f32_total}; }
bool net_info(int net, NetInfo& o) {
    if (net == 0) { o = info_of<NetNerf>(); return true; }
    if (net == 1) { o = info_of<NetNoise>(); return true; }
    return false;
}

// plane code -> number of 16-bit planes stored / computed with
inline bool code_ok(int c) { return (c >= 1 && c <= 3) || c == PLANES_F16; }
inline int nplanes(int c) { return c == PLANES_F16 ? 1 : c; }
constexpr int PT_PAD = 256;     // point arrays are padded to the largest tile (mlp_wide_fwd_kernel: 256 points)
inline long long pad_pts(long long P) { return (P + PT_PAD - 1) / PT_PAD * PT_PAD; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Byte offsets inside the forward stash: [ReLU masks][h_0..][feature][views hidden] with
// `sp` (stash) planes, then the gamma rows with `pf` (forward) planes -- the forward itself
// re-reads them.  sp == 0 (inference) leaves only the gamma rows.
struct StashLayout {
    size_t mask, mask_dummy, pe, xd, h[NET_MAX_LAYERS], feat, hv, total;
    long long Ppad;
};
StashLayout stash_layout(const NetInfo& n, int pf, int sp, long long P) {
    StashLayout L{};
    L.Ppad = pad_pts(P);
    size_t off = 0;
    L.mask = off; off += sp ? al256((size_t)(L.Ppad / 32) * (n.NL + 1) * n.NRB * 16 * 8) : 0;
    L.mask_dummy = off; off += sp ? 4096 : 0;
    for (int l = 0; l < n.NL; ++l) { L.h[l] = off; off += al256((size_t)sp * L.Ppad * n.HW * 2); }
    // the grouped weight-gradient launch (1 and 2 planes) takes the feature layer's gradients from dZv^T h_{NL-1}
    // (FeatFactorArgs): the feature activations are kept for the three-plane reference mode only
    L.feat = off; off += sp >= 3 ? al256((size_t)sp * L.Ppad * n.HW * 2) : 0;
    L.hv = off;   off += al256((size_t)sp * L.Ppad * n.HV * 2);
    L.xd = off;   off += sp ? al256((size_t)L.Ppad * 32) : 0;      // points and view directions (in front of the gamma rows: independent of pf)
    L.pe = off;   off += al256((size_t)pf * L.Ppad * PE_ROW * 2);
    L.total = off;
    return L;
}
struct DStashLayout { size_t scale, fac, dz[NET_MAX_LAYERS], dfeat, dzv, total; };
DStashLayout dstash_layout(const NetInfo& n, int ns, long long P) {
    DStashLayout L{};
    const long long Ppad = pad_pts(P);
    size_t off = 0;
    L.scale = off; off += 256;      // {loss scale, 1/scale, 2 work words} of the fp16 gradient chain, then DW_MAX_JOBS chunk cursors (DwGroup::cursor)
    // 1 and 2 planes: fp32 scratch G = dZv^T h_{NL-1} [HV][HW] then s = sum dZv [HV] (FeatFactorArgs), no d_feature array
    // (one plane: DZV_EXT more rows of G / s for the heads, and the [DZV_EXT][HV] + [DZV_EXT] block of the rgb job)
    L.fac = off; off += ns <= 2 ? al256((size_t)((n.HV + DZV_EXT) * (n.HW + 1) + DZV_EXT * (n.HV + 1)) * 4) : 0;
    for (int l = 0; l < n.NL; ++l) { L.dz[l] = off; off += al256((size_t)ns * Ppad * n.HW * 2); }
    L.dfeat = off; off += ns >= 3 ? al256((size_t)ns * Ppad * n.HW * 2) : 0;
    L.dzv = off;   off += al256((size_t)ns * Ppad * (n.HV + (ns == 1 ? DZV_EXT : 0)) * 2);   // one plane: [dZv | head gradients]
    L.total = off;
    return L;
}

MlpParams to_params(const lush_mlp_params* p) {
    MlpParams q;
    for (int i = 0; i < NET_MAX_LAYERS; ++i) { q.w[i] = p->w[i]; q.b[i] = p->b[i]; }
    q.w_feat = p->w_feat; q.b_feat = p->b_feat; q.w_alpha = p->w_alpha; q.b_alpha = p->b_alpha;
    q.w_views = p->w_views; q.b_views = p->b_views; q.w_rgb = p->w_rgb; q.b_rgb = p->b_rgb;
    return q;
}

// A pack table under construction.  Its jobs come in STREAMS: every segment of one direction in the order a kernel runs them, rows
// permuted by chain_row() or not (`perm`), in consecutive entries from `dst` on; `blocks` runs over the whole table (first_block).
struct PackAdder {
    PackTable& T;
    int& blocks;
    int perm, dst;
    PackAdder(PackTable& t, int& b) : T(t), blocks(b), perm(0), dst(0) { T.n = 0; blocks = 0; }
    PackAdder& stream(int perm_, int dst_) { perm = perm_; dst = dst_; return *this; }
    void add(const float* src, int sr, int sk, int rows, int cols, int nrb, int kk) {
        PackJob& j = T.j[T.n++];
        j.src = src; j.sr = sr; j.sk = sk; j.rows = rows; j.cols = cols; j.nrb = nrb; j.kk = kk; j.perm = perm;
        j.dst_entry = dst; j.first_block = blocks;
        blocks += nrb * kk;
        dst += nrb * kk;
    }
};

// A stream cuts every full-width segment into slices of `slice_rows` rows and runs slice by slice (skip layer: [x part | h part]
// per slice); slice_rows = HW leaves them whole (NetT::fwd_L .. fwd_RGB, bwd_VAT .. bwd_LT are the prefix sums of that order).
// Where the kernels do not agree on the order, the difference is a parameter:
enum ViewsForm {
    VIEWS_WHOLE,                // the views layer uncut: its feature columns, then gamma(d) in KKD k-blocks
    VIEWS_SLICED_DIR_FIRST      // ... in slices too, each [gamma(d) part, K zero-padded to 4 k-blocks (one position) | feature part]
};
enum SkipXOrder { SKIP_X_BEFORE_SLICES, SKIP_X_AFTER_SLICES };   // transposed skip layer: where its 64 gamma(x) rows go

template <class N>
void pack_stream_fwd(PackAdder& A, const lush_mlp_params* p, int slice_rows, ViewsForm views) {
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, SK = N::SKIP;
    const int SR = slice_rows, nrb = SR / 32, XV = PE_X_VALID, DV = PE_D_VALID;
    for (int s = 0; s < HW / SR; ++s) A.add(p->w[0] + (long long)s * SR * XV, XV, 1, SR, XV, nrb, N::KKX);
    for (int l = 1; l < NL; ++l) {
        const int ld = l == SK ? XV + HW : HW;
        for (int s = 0; s < HW / SR; ++s) {
            const float* w = p->w[l] + (long long)s * SR * ld;
            if (l == SK) A.add(w, ld, 1, SR, XV, nrb, N::KKX);
            A.add(w + (l == SK ? XV : 0), ld, 1, SR, HW, nrb, N::KKH);
        }
    }
    for (int s = 0; s < HW / SR; ++s) A.add(p->w_feat + (long long)s * SR * HW, HW, 1, SR, HW, nrb, N::KKH);
    A.add(p->w_alpha, HW, 1, 1, HW, 1, N::KKH);
    if (views == VIEWS_WHOLE) {
        A.add(p->w_views, HW + DV, 1, HV, HW, N::NRBV, N::KKH);
        A.add(p->w_views + HW, HW + DV, 1, HV, DV, N::NRBV, N::KKD);
    } else {
        for (int s = 0; s < HV / SR; ++s) {
            const float* w = p->w_views + (long long)s * SR * (HW + DV);
            A.add(w + HW, HW + DV, 1, SR, DV, nrb, 4);
            A.add(w, HW + DV, 1, SR, HW, nrb, N::KKH);
        }
    }
    A.add(p->w_rgb, HV, 1, 3, HV, 1, N::KKV);
}

// transposed: element (row, k) = W[k][c0 + row]: src = W + c0, row stride 1, k stride = W's row length.
// vbt_kk: k-blocks the gamma(d) segment's K is zero-padded to (NetT::KVB: whole positions of the chain kernels; the 64-points-per-wave
// kernel takes it as one position of KKV)
template <class N>
void pack_stream_bwd(PackAdder& A, const lush_mlp_params* p, int slice_rows, int vbt_kk, SkipXOrder skip_x) {
    constexpr int HW = N::HW, HV = N::HV, NL = N::NL, SK = N::SKIP;
    const int SR = slice_rows, nrb = SR / 32, XV = PE_X_VALID, DV = PE_D_VALID;
    for (int s = 0; s < HW / SR; ++s) A.add(p->w_views + s * SR, 1, HW + DV, SR, HV, nrb, N::KKV);
    A.add(p->w_views + HW, 1, HW + DV, DV, HV, 1, vbt_kk);
    for (int s = 0; s < HW / SR; ++s) A.add(p->w_feat + s * SR, 1, HW, SR, HW, nrb, N::KKH);
    for (int l = NL - 1; l >= 1; --l) {
        const int ld = l == SK ? XV + HW : HW;
        if (l == SK && skip_x == SKIP_X_BEFORE_SLICES) A.add(p->w[l], 1, ld, XV, HW, 2, N::KKH);
        for (int s = 0; s < HW / SR; ++s) A.add(p->w[l] + (l == SK ? XV : 0) + s * SR, 1, ld, SR, HW, nrb, N::KKH);
        if (l == SK && skip_x == SKIP_X_AFTER_SLICES) A.add(p->w[l], 1, ld, XV, HW, 2, N::KKH);
    }
    A.add(p->w[0], 1, XV, XV, HW, 2, N::KKH);
}

// First and second copy in one table, both directions: copy 0 = natural rows (tiled 3-plane kernels: mlp_fwd_kernel,
// mlp_bwd_kernel), copy 1 = chain_row() permutation (chain kernels); segments uncut.
template <class N>
void build_pack_table(const lush_mlp_params* p, PackTable& T, int& blocks, int copy_lo, int copy_hi) {
    PackAdder A(T, blocks);
    for (int copy = copy_lo; copy <= copy_hi; ++copy) pack_stream_fwd<N>(A.stream(copy, copy ? N::fwd2_base : 0), p, N::HW, VIEWS_WHOLE);
    for (int copy = copy_lo; copy <= copy_hi; ++copy)
        pack_stream_bwd<N>(A.stream(copy, copy ? N::bwd2_base : N::bwd_VAT), p, N::HW, N::KVB, SKIP_X_BEFORE_SLICES);
}
// The sliced copies of the 8x256 net, each a table of its own (the kernel argument block holds 64 jobs).  Third copy (NetT::fwd3_base /
// bwd3_base): 128-row halves of mlp_chain_fwd_half_kernel / mlp_chain_bwd_half_kernel; fourth (fwd4_base / bwd4_base): 64-row
// quarters of mlp_wide_fwd_kernel (lush_mlp_wide.hip) / mlp_wide_bwd_kernel (lush_mlp_wide_bwd.hip).
void pack_half_fwd(const lush_mlp_params* p, PackTable& T, int& blocks) { pack_stream_fwd<NetNerf>(PackAdder(T, blocks).stream(1, NetNerf::fwd3_base), p, 128, VIEWS_WHOLE); }
void pack_half_bwd(const lush_mlp_params* p, PackTable& T, int& blocks) { pack_stream_bwd<NetNerf>(PackAdder(T, blocks).stream(1, NetNerf::bwd3_base), p, 128, NetNerf::KVB, SKIP_X_BEFORE_SLICES); }
void pack_wide_fwd(const lush_mlp_params* p, PackTable& T, int& blocks) { pack_stream_fwd<NetNerf>(PackAdder(T, blocks).stream(1, NetNerf::fwd4_base), p, 64, VIEWS_SLICED_DIR_FIRST); }
void pack_wide_bwd(const lush_mlp_params* p, PackTable& T, int& blocks) { pack_stream_bwd<NetNerf>(PackAdder(T, blocks).stream(1, NetNerf::bwd4_base), p, 64, NetNerf::KKV, SKIP_X_AFTER_SLICES); }

// Variant bits by what they select (include/lush_march.h LUSH_VARIANT_*).
// ... an older forward / backward MLP kernel of the one-fp16-plane mode, which reads another copy of the packed weights:
constexpr int OLDER_MLP_KERNEL_VARIANTS = LUSH_VARIANT_FWD_HALF | LUSH_VARIANT_FWD_512 | LUSH_VARIANT_BWD_HALF | LUSH_VARIANT_BWD_512;
// ... a forward that stashes the 256-byte encoded rows (the older forward kernels do; LUSH_VARIANT_PE_ROWS asks for it):
constexpr int ROW_STASH_VARIANTS = LUSH_VARIANT_FWD_HALF | LUSH_VARIANT_FWD_512 | LUSH_VARIANT_PE_ROWS;
// a live-point launch: the 8x256 net's one- and two-plane kernels (the 64-points-per-wave kernels of the one-fp16-plane mode and the
// 128-point-tile chain kernels of the bf16-plane modes, with the grouped weight gradients), no older-kernel variant bit; the
// three-plane reference mode keeps its tiled kernels and the backward over all the points
constexpr int LIVE_OLDER_VARIANTS = OLDER_MLP_KERNEL_VARIANTS | LUSH_VARIANT_PE_ROWS | LUSH_VARIANT_HEAD_KERNEL | LUSH_VARIANT_DW_SPLIT | LUSH_VARIANT_DW_WALK;
bool live_kernels(int net, int planes_f, int planes_b, int variant) {
    return net == 0 && mlp_fwd_chain_enabled(planes_f) && mlp_bwd_chain_enabled(planes_b) && !(variant & LIVE_OLDER_VARIANTS);
}

// The weight gradients of the product's one-fp16-plane kernels re-encode gamma(x), gamma(d) from the 32 bytes per point the forward
// wrote (MlpFwdArgs::xd); every other kernel / variant writes and reads the 256-byte encoded rows (MlpFwdArgs::pe_rows).  Asked by
// the forward and by the weight gradients: the caller passes the same variant word to both.
bool reencodes(int net, int code_fwd, int stash_planes, int variant) {
    return net == 0 && code_fwd == PLANES_F16 && stash_planes == 1 && !(variant & ROW_STASH_VARIANTS);
}

// What must be zero when a grouped weight-gradient launch starts: the chunk queue's cursors in the dstash header (the bytes behind
// the scale and the work words) and the feature-factor scratch behind them.  Zeroed by the loss-scale launch, by a memset, or by
// the caller's compositing backward (mlp_dstash_header) -- all three take the range from here.
struct ZeroRange { float* p; long long n; };       // n floats from p
ZeroRange dstash_zero_range(const DStashLayout& D, const NetInfo& n, void* dstash) {
    return {(float*)((char*)dstash + D.scale + DW_CURSOR_OFF),
            (long long)((D.fac - D.scale - DW_CURSOR_OFF) / 4 + (n.HV + DZV_EXT) * (n.HW + 1) + DZV_EXT * (n.HV + 1))};
}

int device_cus() {      // of the calling thread's device
    int dev = 0, cus = 256;
    if (current_device_cus(dev, cus) != 0) cus = 256;
    return cus;
}

int dw_splits(long long Ppad, int cus) {
    int s = cus;      // one 256x256-tile workgroup per CU
    // every workgroup ends a layer with 256 KB of atomics and starts it with a ring refill: give it at least LUSH_DW_MIN_PTS
    // points (the 4096-point noise net ran 128 workgroups of one tile each: 189 us for 7 tiny GEMMs; 128 points each: 69 us)
#ifndef LUSH_DW_MIN_PTS
#define LUSH_DW_MIN_PTS 128
#endif
    const long long max_s = Ppad / LUSH_DW_MIN_PTS > 0 ? Ppad / LUSH_DW_MIN_PTS : 1;
    if (s > max_s) s = (int)max_s;
    return s < 1 ? 1 : s;
}

// cus workgroups shared out over the jobs in proportion to what a point of each job costs a workgroup (the comment at
// LUSH_VARIANT_DW_SPLIT in plan_dw_group); every job gets at least one
#ifndef LUSH_DW_PE_COST
#define LUSH_DW_PE_COST 860
#endif
void job_shares(const DwGroup& G, int cus, int* nj) {
    long long w[DW_MAX_JOBS], W = 0;
    for (int i = 0; i < G.n; ++i) {
        const DwJob& j = G.j[i];
        const bool pe = j.X2 != nullptr && G.xd != nullptr && j.pe_mode != 0;
        w[i] = 2LL * (j.n_out + j.k_in) + (j.X2 && !pe ? 2LL * j.k2_in : 0);
        if (w[i] < 512) w[i] = 512;
        if (pe) w[i] += 32 + LUSH_DW_PE_COST;
        W += w[i];
    }
    int used = 0;
    double frac[DW_MAX_JOBS];
    for (int i = 0; i < G.n; ++i) {
        const double x = (double)cus * (double)w[i] / (double)W;
        nj[i] = (int)x < 1 ? 1 : (int)x;
        frac[i] = x - (int)x;
        used += nj[i];
    }
    while (used < cus) {                       // the CUs left over go to the jobs that were rounded down the most
        int b = 0;
        for (int i = 1; i < G.n; ++i) if (frac[i] > frac[b]) b = i;
        ++nj[b]; frac[b] = -1.0; ++used;
    }
    while (used > cus) {                       // (only when a narrow job was lifted to one workgroup)
        int b = 0;
        for (int i = 1; i < G.n; ++i) if (nj[i] > nj[b]) b = i;
        --nj[b]; --used;
    }
}

// (b) How a grouped weight-gradient launch is cut up: the form (DwGroup::per_job), the slices (pts_per_split, DwJob::pps, first[]) and
// the grid, from the job table, the padded point count, whether the launch is a live-point one, the variant word and the CU count.
// No HIP call: lush_debug_dw_plan runs it where there is no device.
struct DwPlan {
    int grid_x, grid_y;      // (grid_y is what launch_dw_group makes of per_job: the jobs for 1, else 1)
    bool use_cursor;         // per_job == 3: DwGroup::cursor = the cursors of the dstash header
};
DwPlan plan_dw_group(DwGroup& G, long long Ppad, bool live, int variant, int cus) {
    // A workgroup ends a job with up to 64 K fp32 atomics on addresses every other slice of the job also adds to: ~50 us per
    // job when 256 slices do it at once, whatever the point count (measured: 32 768 points, 11 jobs in turn, 0.55 ms).  Passes
    // below LUSH_DW_PERJOB_MAX_PTS points therefore run ONE job per workgroup (grid: slices x jobs) with just enough slices to
    // fill the chip once -- one round of atomics in all, 1 / slices of the contenders per address (the same pass: 0.15 ms;
    // 4 096 points 0.107 -> 0.064 ms).  Above it a job's streaming time hides its atomics and every workgroup takes every job of
    // its slice in turn, which balances the narrow jobs.
    // (LUSH_DW_PERJOB_MAX_PTS / _MIN_PTS: lush_mlp.h; a live-point launch makes the same choice on the device)
    int splits = dw_splits(Ppad, cus);
    G.per_job = 0;
    if (Ppad <= LUSH_DW_PERJOB_MAX_PTS && !live) {      // (a live-point launch decides in the kernel: its size is known on the device only)
        long long sp = cus / G.n, most = Ppad / LUSH_DW_PERJOB_MIN_PTS;
        if (sp > most) sp = most;
        splits = sp < 1 ? 1 : (int)sp;
        G.per_job = 1;
    }
    long long pps = (Ppad + splits - 1) / splits;
    pps = (pps + 31) / 32 * 32;
    G.Ppad = (int)Ppad;
    G.pts_per_split = (int)pps;
    int grid_x = (int)((Ppad + pps - 1) / pps);
    bool use_cursor = false;
    if (!G.per_job && !live && (variant & LUSH_VARIANT_DW_SPLIT) && cus >= 4 * G.n) {
        // Variant (round 5 experiment, NOT the product's choice: measured slower, see include/lush_march.h): ONE job per
        // workgroup.  A workgroup that walks the ten jobs of its slice drains its ring,
        // flushes 40 K atomics, zeroes and refills the ring ten times -- the launch averaged 86 % of its own streaming rate.
        // Here job j gets n_j of the chip's workgroups, n_j proportional to what a point of that job costs a workgroup, and
        // slices of Ppad / n_j points: every workgroup is busy for the same time and has ONE boundary.  The grid is flat,
        // sum n_j = CUs workgroups: every one is resident from the start.
        // Cost per point, in bytes-equivalent (profiles/r05_dw_jobs.md: per-workgroup durations of a byte-proportional
        // split, -DLUSH_CLOCK): the bytes the job streams (Z row + X row), at least 512 (a narrow job is latency-bound: three
        // small stages in flight), plus DW_PE_COST for a block that is re-encoded from the 32-byte point record (the
        // encoding's ~150 VALU instructions per stage run on four of the eight waves: 27 ns per point).
        int nj[DW_MAX_JOBS];
        job_shares(G, cus, nj);
        grid_x = 0;
        for (int i = 0; i < G.n; ++i) {
            long long p = (Ppad + nj[i] - 1) / nj[i];
            p = (p + 31) / 32 * 32;
            G.j[i].pps = (int)p;
            G.first[i] = grid_x;
            grid_x += (int)((Ppad + p - 1) / p);
        }
        G.first[G.n] = grid_x;
        G.per_job = 2;
    }
    if (!G.per_job && Ppad > LUSH_DW_PERJOB_MAX_PTS && !(variant & LUSH_VARIANT_DW_WALK) && grid_x >= 2 * G.n) {
        // The product's choice above LUSH_DW_PERJOB_MAX_PTS points, dense and live (a live launch whose list turns out shorter
        // falls back to one job per workgroup in the kernel, as before): the chunk queue (DwGroup::per_job == 3).  The walk paid
        // ten drain / flush / zero / refill boundaries per workgroup whatever the point count (profiles/r07_dw_queue.md);
        // here a workgroup flushes when the job it streams runs out of chunks.  The cursors are zero: they lie in the dstash
        // header, which is zeroed together with the feature-factor scratch behind it (dstash_zero_range).
        int nj[DW_MAX_JOBS];
        job_shares(G, grid_x, nj);
        G.first[0] = 0;
        for (int i = 0; i < G.n; ++i) G.first[i + 1] = G.first[i] + nj[i];
        use_cursor = true;
        G.per_job = 3;
    }
    return {grid_x, G.per_job == 1 ? G.n : 1, use_cursor};
}

}  // namespace

extern "C" {

size_t lush_mlp_packed_bytes(int net, int planes) {
    NetInfo n;
    if (!net_info(net, n) || !code_ok(planes)) return 0;
    return al256((size_t)n.total_entries * nplanes(planes) * 1024 + (size_t)n.f32_total * 4);
}

// The fragment tables one (net, plane code, variant) needs, in launch order: what lush_mlp_pack / lush_mlp_pack_for launch
// one by one and a pack plan (lush_pack_plan_*) holds as one table.  variant < 0: every copy.
static int collect_pack_tables(int net, int planes, const lush_mlp_params* prm, int variant, std::vector<PackTable>& out,
                               std::vector<int>& out_blocks) {
    if (!code_ok(planes)) return set_error("lush_mlp_pack: planes must be 1..3 or 17 (fp16)");
    if (net != 0 && net != 1) return set_error("lush_mlp_pack: bad net");
    auto push = [&](const PackTable& T, int blocks) { out.push_back(T); out_blocks.push_back(blocks); };
    PackTable T;
    int blocks = 0;
    // the product's kernels for one fp16 plane on the 8x256 net read the two quarter-row streams and the fp32 block only:
    // three launches instead of six (the launch-bound configurations pay for every one of them)
    if (net == 0 && planes == PLANES_F16 && variant >= 0 && !(variant & OLDER_MLP_KERNEL_VARIANTS)) {
        pack_wide_fwd(prm, T, blocks);
        if (blocks != NetNerf::fwd4_len) return set_error("lush_mlp_pack: quarter-row stream length");
        push(T, blocks);
        pack_wide_bwd(prm, T, blocks);
        if (blocks != NetNerf::bwd4_len) return set_error("lush_mlp_pack: transposed quarter-row stream length");
        push(T, blocks);
        return 0;
    }
    // only the copies the kernels of this plane count read (the rest of the buffer stays unwritten)
    const bool fc = mlp_fwd_chain_enabled(planes), bc = mlp_bwd_chain_enabled(planes);
    const int lo = (fc && bc) ? 1 : 0, hi = (fc || bc) ? 1 : 0;
    if (net == 0) build_pack_table<NetNerf>(prm, T, blocks, lo, hi);
    else build_pack_table<NetNoise>(prm, T, blocks, lo, hi);
    push(T, blocks);
    if (net == 0 && nplanes(planes) == 1) {      // the half-row streams are read by the one-plane chain kernels only
        pack_half_fwd(prm, T, blocks);
        push(T, blocks);
        if (planes == PLANES_F16) {              // ... and the half-row backward by the fp16 chain only
            pack_half_bwd(prm, T, blocks);
            push(T, blocks);
            pack_wide_fwd(prm, T, blocks);     // quarter-row forward stream (64 points per wave)
            if (blocks != NetNerf::fwd4_len) return set_error("lush_mlp_pack: quarter-row stream length");
            push(T, blocks);
            pack_wide_bwd(prm, T, blocks);     // ... and its transposed twin
            if (blocks != NetNerf::bwd4_len) return set_error("lush_mlp_pack: transposed quarter-row stream length");
            push(T, blocks);
        }
    }
    return 0;
}

int lush_mlp_pack_for(int net, int planes, const lush_mlp_params* prm, void* packed, int variant, lush_stream_t stream) {
    std::vector<PackTable> tables;
    std::vector<int> blocks;
    int rc = collect_pack_tables(net, planes, prm, variant, tables, blocks);
    for (size_t i = 0; i < tables.size() && !rc; ++i) rc = launch_pack(planes, tables[i], blocks[i], packed, (hipStream_t)stream);
    if (rc) return rc;
    return launch_pack_f32(net, nplanes(planes), to_params(prm), packed, (hipStream_t)stream);
}

int lush_mlp_pack(int net, int planes, const lush_mlp_params* prm, void* packed, lush_stream_t stream) {
    return lush_mlp_pack_for(net, planes, prm, packed, -1, stream);
}

// ---- pack plans: every network of a training step in ONE launch ----
size_t lush_pack_plan_bytes(int n_jobs) {
    if (n_jobs < 1 || n_jobs > PLAN_MAX_NETS) return 0;
    return al256(sizeof(PlanHeader) + sizeof(MlpParams) * PLAN_MAX_NETS + sizeof(PlanJob) * (size_t)n_jobs * 260);
}

int lush_pack_plan_build(const lush_pack_job* jobs, int n_jobs, void* plan, size_t plan_bytes, int* launch_blocks) {
    if (!jobs || !plan || !launch_blocks) return set_error("lush_pack_plan_build: jobs, plan and launch_blocks are required");
    if (n_jobs < 1 || n_jobs > PLAN_MAX_NETS) return set_error("lush_pack_plan_build: 1 .. 8 jobs");
    std::vector<PlanJob> pj;
    std::vector<MlpParams> prms(PLAN_MAX_NETS);
    int total = 0;
    for (int k = 0; k < n_jobs; ++k) {
        const lush_pack_job& J = jobs[k];
        if (!J.prm || !J.packed) return set_error("lush_pack_plan_build: a job without parameters or destination");
        std::vector<PackTable> tables;
        std::vector<int> blocks;
        int rc = collect_pack_tables(J.net, J.planes, J.prm, J.variant, tables, blocks);
        if (rc) return rc;
        for (size_t t = 0; t < tables.size(); ++t) {
            for (int i = 0; i < tables[t].n; ++i) {
                PlanJob q{};
                q.j = tables[t].j[i];
                q.j.first_block += total;
                q.dst = J.packed; q.code = J.planes; q.kind = 0; q.prm_index = k;
                pj.push_back(q);
            }
            total += blocks[t];
        }
        prms[k] = to_params(J.prm);
        PlanJob f{};
        const int f32_total = J.net == 0 ? NetNerf::f32_total : NetNoise::f32_total;
        const int entries = J.net == 0 ? NetNerf::total_entries : NetNoise::total_entries;
        f.j.first_block = total;
        f.dst = reinterpret_cast<float*>(J.packed) + (size_t)entries * nplanes(J.planes) * 256;
        f.code = J.planes; f.kind = J.net == 0 ? 1 : 2; f.prm_index = k;
        pj.push_back(f);
        total += (f32_total + 63) / 64;
    }
    const size_t need = sizeof(PlanHeader) + sizeof(MlpParams) * PLAN_MAX_NETS + sizeof(PlanJob) * pj.size();
    if (need > plan_bytes) return set_error("lush_pack_plan_build: plan buffer too small (lush_pack_plan_bytes)");
    std::vector<char> host(need);
    PlanHeader H{(int)pj.size(), total, n_jobs, 0};
    memcpy(host.data(), &H, sizeof(H));
    memcpy(host.data() + sizeof(H), prms.data(), sizeof(MlpParams) * PLAN_MAX_NETS);
    memcpy(host.data() + sizeof(H) + sizeof(MlpParams) * PLAN_MAX_NETS, pj.data(), sizeof(PlanJob) * pj.size());
    LUSH_HIP(hipMemcpy(plan, host.data(), need, hipMemcpyHostToDevice));       // (set-up call: synchronous, once per model)
    *launch_blocks = total;
    return 0;
}

int lush_pack_plan_run(const void* plan, int launch_blocks, float* zero_buf, long long zero_n, lush_stream_t stream) {
    if (!plan || launch_blocks < 1) return set_error("lush_pack_plan_run: no plan");
    if (zero_n < 0 || (zero_n > 0 && !zero_buf)) return set_error("lush_pack_plan_run: bad zero buffer");
    return launch_pack_plan(plan, launch_blocks, (hipStream_t)stream, zero_n > 0 ? zero_buf : nullptr, zero_n);
}

size_t lush_mlp_stash_bytes(int net, int planes_fwd, int stash_planes, long long P) {
    NetInfo n;
    if (!net_info(net, n) || !code_ok(planes_fwd) || stash_planes < 0 || nplanes(stash_planes) > nplanes(planes_fwd)) return 0;
    // inference on the chain kernel keeps the encoding image in LDS and touches no workspace at all
    if (stash_planes == 0 && mlp_fwd_chain_enabled(planes_fwd)) return 256;
    return stash_layout(n, nplanes(planes_fwd), nplanes(stash_planes), P).total;
}
size_t lush_mlp_dstash_bytes(int net, int planes, long long P) {
    NetInfo n;
    if (!net_info(net, n) || !code_ok(planes)) return 0;
    return dstash_layout(n, nplanes(planes), P).total;
}

int lush_debug_stash_layout(int net, int planes, long long P, long long* o) {
    NetInfo n;
    if (!net_info(net, n)) return set_error("bad net");
    const StashLayout L = stash_layout(n, planes, planes, P);
    o[0] = (long long)L.mask; o[1] = (long long)L.pe;
    for (int l = 0; l < NET_MAX_LAYERS; ++l) o[2 + l] = l < n.NL ? (long long)L.h[l] : -1;
    o[10] = (long long)L.feat; o[11] = (long long)L.hv; o[12] = L.Ppad; o[13] = (long long)L.total;
    o[14] = n.HW; o[15] = n.NL;
    return 0;
}

}  // extern "C"

namespace {

// ---- the forward ----
// (in the order of lush_mlp_fwd's parameters; live_idx / live_cnt both null: a launch over all the points, which writes `raw`)
struct FwdRequest {
    int net, planes, stash_planes; const float *rays, *z; int R, S; const void* packed; float* raw; void* stash; int variant;
    lush_stream_t stream; const int *live_idx, *live_cnt;
    bool trunk_only;      // lush_mlp_fwd_trunk: layers 0 .. 7 and the alpha head, raw = (0, 0, 0, sigma)
};
int mlp_fwd(const FwdRequest& q) {
    const int net = q.net, planes = q.planes;
    int stash_planes = q.stash_planes;
    NetInfo n;
    if (!net_info(net, n)) return set_error("lush_mlp_fwd: bad net");
    if (!code_ok(planes)) return set_error("lush_mlp_fwd: planes must be 1..3 or 17 (one fp16 plane)");
    if (stash_planes == PLANES_F16) stash_planes = 1;
    if (stash_planes < 0 || stash_planes > nplanes(planes)) return set_error("lush_mlp_fwd: need 0 <= stash_planes <= planes");
    if (!q.stash) return set_error("lush_mlp_fwd: stash (or the inference workspace) is required");
    if (q.R <= 0 || q.S <= 0) return set_error("lush_mlp_fwd: empty batch");
    const long long P = (long long)q.R * q.S;
    // the 64-points-per-wave kernels address d_raw / the point rows by 32-bit byte offsets from a scalar base (16 .. 32 bytes per
    // point): one launch takes at most 2^27 - 1 points (whose stash alone would be 590 GB); split the rays above that
    if (P >= (1LL << 27)) return set_error("lush_mlp_fwd: at most 2^27 - 1 points per launch (split the ray batch)");
    const StashLayout L = stash_layout(n, nplanes(planes), stash_planes, P);
    const bool chain = mlp_fwd_chain_enabled(planes);
    const int mt = chain ? 128 : (planes == PLANES_F16 ? 64 : mlp_fwd_tile(planes));
    MlpFwdArgs a{};
    a.stash_planes = stash_planes;
    a.rays = q.rays; a.z = q.z; a.S = q.S; a.P = (int)P; a.n_tiles = (int)(L.Ppad / mt);
    a.wpk = (const uint4*)q.packed;              // (the biases travel inside `packed`, lush_mlp_pack: the fp32 parameters are not read)
    a.raw = q.raw;
    a.write_stash = stash_planes > 0;
    char* b = (char*)q.stash;
    a.mask = (unsigned long long*)(b + L.mask);
    a.mask_dummy = b + L.mask_dummy;
    a.pe = (__bf16*)(b + L.pe);
    a.xd = (float*)(b + L.xd);
    a.pe_rows = !reencodes(net, planes, stash_planes, q.variant);
    a.h0 = (__bf16*)(b + L.h[0]);
    a.h_stride = n.NL > 1 ? (long long)(L.h[1] - L.h[0]) / 2 : 0;
    a.feat = (__bf16*)(b + L.feat);
    a.hv = (__bf16*)(b + L.hv);
    a.plane_pe = L.Ppad * PE_ROW; a.plane_h = L.Ppad * n.HW; a.plane_hv = L.Ppad * n.HV;
    a.live_idx = q.live_idx; a.live_cnt = q.live_cnt;
    if (q.live_idx || q.live_cnt) {
        if (!q.live_idx || !q.live_cnt) return set_error("lush_mlp_fwd_live: the list and its count come together");
        if (net != 0 || !chain || (q.variant & LIVE_OLDER_VARIANTS) || stash_planes < 1) return set_error("lush_mlp_fwd_live: the 8x256 net's one- or two-plane kernels with the stash, no older-kernel variant");
        // (only the 64-points-per-wave kernel writes the rows of a live-point launch)
        if (q.raw && (planes != PLANES_F16 || stash_planes != 1)) return set_error("lush_mlp_fwd_live_raw: one fp16 plane with its stash");
    }
    if (q.trunk_only) {
        if (net != 0 || planes != PLANES_F16 || stash_planes != 0 || (q.variant & (LUSH_VARIANT_FWD_HALF | LUSH_VARIANT_FWD_512)) || q.live_idx || !q.raw)
            return set_error("lush_mlp_fwd_trunk: the 8x256 net's one-fp16-plane 64-points-per-wave kernel over all the points, no stash, no older-kernel variant");
        a.trunk_only = 1;
    }
    if (chain) return launch_mlp_chain_fwd(net, planes, a, q.variant, (hipStream_t)q.stream);
    const int grid = a.n_tiles < 1024 ? a.n_tiles : 1024;
    return launch_mlp_fwd(net, planes, a, grid, (hipStream_t)q.stream);
}

// ---- the backward ----
// What a backward call asks for: bwd_pass() takes what every call has, chain() / weights() add the half (or both halves) wanted
// and what only that half reads, live() the live-point list, prepared() says that the caller's lush_composite_bwd already computed
// the loss scale into the dstash header and zeroed the cursors and the feature-factor scratch behind it (lush_march_bwd: no
// memset, no grad_scale launch here).
struct BwdRequest {
    int net, planes_f, planes_b, R, S, variant;
    const lush_mlp_params* prm; const float* draw; const void* stash; void* dstash; lush_stream_t stream;
    bool do_chain, do_weights, is_prepared;
    const float *rays, *z; const void* packed_b; float* dpts;      // the chain's
    const lush_mlp_grads* g;                                        // the weight gradients'
    const int *live_idx, *live_cnt;
    BwdRequest& chain(const float* r, const float* z_, const void* pk, float* d) { do_chain = true; rays = r; z = z_; packed_b = pk; dpts = d; return *this; }
    BwdRequest& weights(const lush_mlp_grads* g_) { do_weights = true; g = g_; return *this; }
    BwdRequest& live(const int* idx, const int* cnt) { live_idx = idx; live_cnt = cnt; return *this; }
    BwdRequest& prepared() { is_prepared = true; return *this; }
};
BwdRequest bwd_pass(int net, int planes_f, int planes_b, int R, int S, const lush_mlp_params* prm, const float* draw, const void* stash,
                    void* dstash, int variant, lush_stream_t stream) {
    return {net, planes_f, planes_b, R, S, variant, prm, draw, stash, dstash, stream, false, false, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
}

// What both halves work from, built once per call: the checked plane counts, the two layouts and the chain's argument block.
struct BwdCtx {
    NetInfo n;
    int planes_f, planes_b, code_b;      // plane COUNTS (PLANES_F16 counts as one) and the backward's plane code
    bool x_f16, z_f16, chain;            // the stash was written by the fp16 forward; loss-scaled fp16 gradient chain (one plane); chain kernels
    long long P;
    StashLayout L; DStashLayout D;
    const char* sb; char* db;            // stash, dstash
    hipStream_t st;
    float* gscale;                       // {loss scale, 1/scale} in the dstash header (fp16 chain), or null
    __bf16* dzp[NET_MAX_LAYERS];
    MlpBwdArgs a;
    const __bf16* at(size_t off) const { return (const __bf16*)(sb + off); }
    const __bf16* H(int l) const { return at(L.h[l]); }
    const __bf16* pe() const { return at(L.pe); }
    const __bf16* feat() const { return at(L.feat); }
    const __bf16* hv() const { return at(L.hv); }
};

int bwd_context(const BwdRequest& q, BwdCtx& c) {
    if (!net_info(q.net, c.n)) return set_error("lush_mlp_bwd: bad net");
    const NetInfo& n = c.n;
    if (q.live_cnt && !live_kernels(q.net, q.planes_f, q.planes_b, q.variant)) return set_error("lush_mlp_bwd (live points): the 8x256 net's one- or two-plane kernels, no older-kernel variant");
    c.x_f16 = q.planes_f == PLANES_F16; c.planes_f = c.x_f16 ? 1 : q.planes_f;
    c.z_f16 = q.planes_b == PLANES_F16; c.planes_b = c.z_f16 ? 1 : q.planes_b; c.code_b = q.planes_b;
    if (c.planes_b < 1 || c.planes_b > c.planes_f || c.planes_f > 3) return set_error("lush_mlp_bwd: need 1 <= planes_b <= planes_f <= 3");
    if (!q.stash || !q.dstash) return set_error("lush_mlp_bwd: stash and dstash are required");
    c.P = (long long)q.R * q.S;
    if (q.R <= 0 || q.S <= 0 || c.P >= (1LL << 27)) return set_error("lush_mlp_bwd: 1 .. 2^27 - 1 points per launch (32-bit byte offsets; split the ray batch)");
    c.L = stash_layout(n, c.planes_f, c.planes_f, c.P);   // gamma rows come last: their plane count does not move the others
    c.D = dstash_layout(n, c.planes_b, c.P);
    c.st = (hipStream_t)q.stream; c.sb = (const char*)q.stash; c.db = (char*)q.dstash;
    c.chain = mlp_bwd_chain_enabled(c.code_b);
    if (c.z_f16 && !c.chain) return set_error("lush_mlp_bwd: the fp16 gradient chain needs the chain kernels");
    c.gscale = c.z_f16 ? (float*)(c.db + c.D.scale) : nullptr;
    for (int l = 0; l < n.NL; ++l) c.dzp[l] = (__bf16*)(c.db + c.D.dz[l]);
    MlpBwdArgs& a = c.a = MlpBwdArgs{};
    a.scale = c.gscale;
    a.rays = q.rays; a.z = q.z; a.S = q.S; a.P = (int)c.P; a.n_tiles = (int)(c.L.Ppad / (c.chain ? 128 : mlp_bwd_tile(c.planes_b)));
    a.wpk = (const uint4*)q.packed_b;
    a.draw = q.draw;
    a.mask = (const unsigned long long*)(c.sb + c.L.mask);
    a.dz0 = c.dzp[0];
    a.dz_stride = n.NL > 1 ? (long long)(c.D.dz[1] - c.D.dz[0]) / 2 : 0;
    a.dfeat = (__bf16*)(c.db + c.D.dfeat);
    a.dzv = (__bf16*)(c.db + c.D.dzv);
    a.plane_h = c.L.Ppad * n.HW; a.plane_hv = c.L.Ppad * n.HV;
    a.dpts = q.dpts;
    a.live_idx = q.live_idx; a.live_cnt = q.live_cnt;
    return 0;
}

// The gradient chain (and, for the fp16 chain of a caller that did not prepare the header, its loss scale first).
// fac_zeroed: the loss-scale launch also zeroed what the grouped weight gradients need zero (dstash_zero_range).
int bwd_chain(const BwdRequest& q, const BwdCtx& c, bool& fac_zeroed) {
    if (c.z_f16 && !q.is_prepared) {
        if (!q.draw) return set_error("lush_mlp_bwd: draw is required");
        // (chain and weight gradients in ONE call -- the noise net's backward: the loss-scale launch also zeroes the scratch the
        // grouped launch accumulates into, instead of a fill launch of its own)
        fac_zeroed = q.do_weights && c.planes_b <= 2;
        const ZeroRange zr = fac_zeroed ? dstash_zero_range(c.D, c.n, c.db) : ZeroRange{nullptr, 0};
        const int rc = launch_grad_scale(q.draw, c.P * 4, c.gscale, zr.p, zr.n, c.st);
        if (rc) return rc;
    }
    if (c.chain) return launch_mlp_chain_bwd(q.net, c.code_b, c.a, q.variant, c.st);
    return launch_mlp_bwd(q.net, c.planes_b, c.a, c.a.n_tiles < 1024 ? c.a.n_tiles : 1024, c.st);
}

// (a) The job table of the one grouped launch (1 and 2 planes): every layer of the pass, the two pairs that share a dZ merged
// (DwJob::X2), and the arguments of the feature-factor kernel that finishes its last jobs (F.Hd set: the heads rode along).
// How the launch is cut up is plan_dw_group's business.
int dw_job_table(const BwdRequest& q, const BwdCtx& c, DwGroup& G, FeatFactorArgs& F) {
    const NetInfo& n = c.n;
    const lush_mlp_grads* g = q.g;
    const int XV = PE_X_VALID, DV = PE_D_VALID;
    auto job = [&](const __bf16* Z, int ldz, int n_out, const __bf16* X, int ldx, int xcol0, int k_in, float* dW,
                   int ldw, int wcol0, float* dbias) -> DwJob& {
        DwJob& j = G.j[G.n++];
        j.Z = Z; j.ldz = ldz; j.n_out = n_out; j.X = X; j.ldx = ldx; j.xcol0 = xcol0; j.k_in = k_in;
        j.X2 = nullptr; j.ldx2 = 0; j.x2col0 = 0; j.k2_in = 0;
        j.z_plane = (long long)c.L.Ppad * ldz; j.x_plane = (long long)c.L.Ppad * ldx; j.x2_plane = 0;
        j.dW = dW; j.ldw = ldw; j.wcol0 = wcol0; j.dW2 = dW; j.ldw2 = ldw; j.wcol2 = 0; j.n_out2 = n_out; j.db = dbias;
        j.pe_mode = 0;
        return j;
    };
    const bool reencode = reencodes(q.net, c.x_f16 ? PLANES_F16 : c.planes_f, c.planes_b, q.variant);
    G.xd = reencode ? (const float*)(c.sb + c.L.xd) : nullptr;
    G.live_cnt = q.live_cnt;
    G.scale = c.gscale;
    auto with_pe = [&](DwJob& j, int col0, int k2, float* dW2, int ldw2, int wcol2) {
        j.X2 = c.pe(); j.ldx2 = PE_ROW; j.x2col0 = col0; j.k2_in = k2; j.x2_plane = c.L.Ppad * PE_ROW;
        j.dW2 = dW2; j.ldw2 = ldw2; j.wcol2 = wcol2;
        j.pe_mode = col0 == 0 ? 1 : 2;
    };
    for (int l = 0; l < n.NL; ++l) {
        if (l == 0 && reencode) {      // no rows to stream: the encoding is the job's second input block, computed in the kernel
            DwJob& j = job(c.dzp[0], n.HW, n.HW, nullptr, PE_ROW, 0, 0, g->w[0], XV, 0, g->b[0]);
            with_pe(j, 0, XV, g->w[0], XV, 0);
        } else if (l == 0) {
            job(c.dzp[0], n.HW, n.HW, c.pe(), PE_ROW, 0, XV, g->w[0], XV, 0, g->b[0]);
        } else if (l == n.SKIP) {
            DwJob& j = job(c.dzp[l], n.HW, n.HW, c.H(l - 1), n.HW, 0, n.HW, g->w[l], XV + n.HW, XV, g->b[l]);
            with_pe(j, 0, XV, g->w[l], XV + n.HW, 0);
        } else {
            job(c.dzp[l], n.HW, n.HW, c.H(l - 1), n.HW, 0, n.HW, g->w[l], n.HW, 0, g->b[l]);
        }
    }
    // feature + views layers: G = dZv^T h_{NL-1} and s = sum dZv into scratch (launch_feat_factor turns them
    // into dW_feat, db_feat, dW_views[:, :HW], db_views); the gamma(d) columns of dW_views directly
    if (!q.prm || !q.prm->w_views || !q.prm->w_feat || !q.prm->b_feat) return set_error("lush_mlp_bwd: the grouped weight gradients need the fp32 parameters");
    // One plane: the K<=3 heads ride along (DZV_EXT in lush_mlp.h) unless the caller asks for the separate head kernel.
    const bool fold = c.planes_b == 1 && !(q.variant & LUSH_VARIANT_HEAD_KERNEL);
    const bool alpha = q.net == 0 && g->w_alpha != nullptr && g->b_alpha != nullptr;     // (the noise net's alpha head has no gradient)
    const int ldzv = n.HV + (c.planes_b == 1 ? DZV_EXT : 0), grow = n.HV + DZV_EXT;
    float* facG = (float*)(c.db + c.D.fac);              // [grow][HW]
    float* facS = facG + (size_t)grow * n.HW;            // [grow]
    float* facH = facS + grow;                           // [DZV_EXT][HV]
    float* facSH = facH + (size_t)DZV_EXT * n.HV;        // [DZV_EXT]
    {
        DwJob& j = job(c.a.dzv, ldzv, fold && alpha ? grow : n.HV, c.H(n.NL - 1), n.HW, 0, n.HW, facG, n.HW, 0, facS);
        with_pe(j, PE_X, DV, g->w_views, n.HW + DV, n.HW);
        j.n_out2 = n.HV;
    }
    if (fold) job(c.a.dzv + n.HV, ldzv, DZV_EXT, c.hv(), n.HV, 0, n.HV, facH, n.HV, 0, facSH);   // rgb head: Z = the extra columns, X = views hidden
    F.G = facG; F.s = facS;
    if (fold) {
        F.Hd = facH; F.sH = facSH; F.g_w_rgb = g->w_rgb; F.g_b_rgb = g->b_rgb;
        F.g_w_alpha = alpha ? g->w_alpha : nullptr; F.g_b_alpha = alpha ? g->b_alpha : nullptr;
    }
    F.w_views = q.prm->w_views; F.w_feat = q.prm->w_feat; F.b_feat = q.prm->b_feat;
    F.g_w_feat = g->w_feat; F.g_b_feat = g->b_feat; F.g_w_views = g->w_views; F.g_b_views = g->b_views;
    F.HW = n.HW; F.HV = n.HV; F.ldv = n.HW + DV;
    return 0;
}

// (c) The launches of the grouped path: the grouped launch, the feature-factor kernel behind it, and the head kernel when the
// heads did not ride along.
int bwd_weights_grouped(const BwdRequest& q, const BwdCtx& c, bool fac_zeroed) {
    DwGroup G{};
    FeatFactorArgs F{};
    int rc = dw_job_table(q, c, G, F);
    if (rc) return rc;
    if (!q.is_prepared && !fac_zeroed) {
        const ZeroRange zr = dstash_zero_range(c.D, c.n, c.db);
        LUSH_HIP(hipMemsetAsync(zr.p, 0, (size_t)zr.n * 4, c.st));
    }
    const DwPlan plan = plan_dw_group(G, c.L.Ppad, q.live_cnt != nullptr, q.variant, device_cus());
    if (plan.use_cursor) G.cursor = (int*)(c.db + c.D.scale + DW_CURSOR_OFF);
    rc = launch_dw_group(G, plan.grid_x, c.planes_b, c.x_f16, c.z_f16, c.st);
    if (rc) return rc;
    rc = launch_feat_factor(F, c.st);
    if (rc || F.Hd) return rc;
    return launch_head_dw(c.planes_b, c.x_f16, q.draw, c.P, c.hv(), c.a.plane_hv, c.n.HV, c.H(c.n.NL - 1), c.a.plane_h, c.n.HW, q.g->w_rgb, q.g->b_rgb,
                          q.net == 0 ? q.g->w_alpha : nullptr, q.net == 0 ? q.g->b_alpha : nullptr, c.st, q.live_cnt);
}

// three planes (test reference): one launch per layer
int bwd_weights_per_layer(const BwdRequest& q, const BwdCtx& c) {
    const NetInfo& n = c.n;
    const lush_mlp_grads* g = q.g;
    const int XV = PE_X_VALID, DV = PE_D_VALID;
    const int splits = dw_splits(c.L.Ppad, device_cus());
    long long pps = (c.L.Ppad + splits - 1) / splits;
    pps = (pps + 31) / 32 * 32;
    const int real_splits = (int)((c.L.Ppad + pps - 1) / pps);
    // Z [plane][Ppad][ldz], X [plane][Ppad][ldx]
    auto dw = [&](const __bf16* Z, int ldz, int n_out, const __bf16* X, int ldx, int xcol0, int k_in, float* dW, int ldw, int wcol0,
                  float* dbias) {
        DwArgs d{};
        d.Z = Z; d.z_plane = c.L.Ppad * ldz; d.ldz = ldz; d.n_out = n_out;
        d.X = X; d.x_plane = c.L.Ppad * ldx; d.ldx = ldx; d.xcol0 = xcol0; d.k_in = k_in;
        d.dW = dW; d.ldw = ldw; d.wcol0 = wcol0; d.db = dbias;
        d.x_f16 = c.x_f16 ? 1 : 0;
        d.z_f16 = c.z_f16 ? 1 : 0;
        d.scale = c.gscale;
        d.Ppad = (int)c.L.Ppad;
        d.pts_per_split = (int)pps;
        return launch_dw(c.planes_b, d, real_splits, c.st);
    };
    int rc = 0;
    for (int l = 0; l < n.NL && !rc; ++l) {
        const __bf16* Z = c.dzp[l];
        if (l == 0) {
            rc = dw(Z, n.HW, n.HW, c.pe(), PE_ROW, 0, XV, g->w[0], XV, 0, g->b[0]);
        } else if (l == n.SKIP) {
            rc = dw(Z, n.HW, n.HW, c.pe(), PE_ROW, 0, XV, g->w[l], XV + n.HW, 0, g->b[l]);
            if (!rc) rc = dw(Z, n.HW, n.HW, c.H(l - 1), n.HW, 0, n.HW, g->w[l], XV + n.HW, XV, nullptr);
        } else {
            rc = dw(Z, n.HW, n.HW, c.H(l - 1), n.HW, 0, n.HW, g->w[l], n.HW, 0, g->b[l]);
        }
    }
    if (rc) return rc;
    rc = dw(c.a.dfeat, n.HW, n.HW, c.H(n.NL - 1), n.HW, 0, n.HW, g->w_feat, n.HW, 0, g->b_feat);
    if (rc) return rc;
    rc = dw(c.a.dzv, n.HV, n.HV, c.feat(), n.HW, 0, n.HW, g->w_views, n.HW + DV, 0, g->b_views);
    if (rc) return rc;
    rc = dw(c.a.dzv, n.HV, n.HV, c.pe(), PE_ROW, PE_X, DV, g->w_views, n.HW + DV, n.HW, nullptr);
    if (rc) return rc;
    return launch_head_dw(c.planes_b, c.x_f16, q.draw, c.P, c.hv(), c.a.plane_hv, n.HV, c.H(n.NL - 1), c.a.plane_h, n.HW, g->w_rgb, g->b_rgb,
                          q.net == 0 ? g->w_alpha : nullptr, q.net == 0 ? g->b_alpha : nullptr, c.st);
}

int mlp_bwd(const BwdRequest& q) {
    BwdCtx c;
    int rc = bwd_context(q, c);
    if (rc) return rc;
    bool fac_zeroed = false;
    if (q.do_chain) rc = bwd_chain(q, c, fac_zeroed);
    if (rc || !q.do_weights) return rc;
    return c.planes_b <= 2 ? bwd_weights_grouped(q, c, fac_zeroed) : bwd_weights_per_layer(q, c);
}

}  // namespace

extern "C" {

int lush_mlp_fwd(int net, int planes, int stash_planes, const float* rays, const float* z, int R, int S,
                 const void* packed, const lush_mlp_params*, float* raw, void* stash, int variant, lush_stream_t stream) {
    return mlp_fwd({net, planes, stash_planes, rays, z, R, S, packed, raw, stash, variant, stream, nullptr, nullptr});
}
int lush_mlp_fwd_live(int net, int planes, int stash_planes, const float* rays, const float* z, int R, int S, const void* packed,
                      const lush_mlp_params*, void* stash, const int* live_idx, const int* live_cnt, int variant, lush_stream_t stream) {
    if (!live_idx || !live_cnt) return set_error("lush_mlp_fwd_live: live_idx and live_cnt are required");
    return mlp_fwd({net, planes, stash_planes, rays, z, R, S, packed, nullptr, stash, variant, stream, live_idx, live_cnt});
}

int lush_mlp_fwd_live_raw(int net, int planes, int stash_planes, const float* rays, const float* z, int R, int S, const void* packed,
                          void* stash, const int* live_idx, const int* live_cnt, float* raw, int variant, lush_stream_t stream) {
    if (!live_idx || !live_cnt) return set_error("lush_mlp_fwd_live_raw: live_idx and live_cnt are required");
    return mlp_fwd({net, planes, stash_planes, rays, z, R, S, packed, raw, stash, variant, stream, live_idx, live_cnt});
}
int lush_mlp_fwd_trunk(int net, int planes, const float* rays, const float* z, int R, int S, const void* packed, float* raw,
                       void* workspace, int variant, lush_stream_t stream) {
    return mlp_fwd({net, planes, 0, rays, z, R, S, packed, raw, workspace, variant, stream, nullptr, nullptr, true});
}

int lush_mlp_bwd(int net, int planes_f, int planes_b, const float* rays, const float* z, int R, int S,
                 const void* packed_b, const lush_mlp_params* prm, const float* draw, const void* stash,
                 void* dstash, const lush_mlp_grads* g, float* dpts, int variant, lush_stream_t stream) {
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw, stash, dstash, variant, stream).chain(rays, z, packed_b, dpts).weights(g));
}
int lush_mlp_bwd_chain(int net, int planes_f, int planes_b, const float* rays, const float* z, int R, int S,
                       const void* packed_b, const lush_mlp_params* prm, const float* draw, const void* stash,
                       void* dstash, float* dpts, int variant, lush_stream_t stream) {
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw, stash, dstash, variant, stream).chain(rays, z, packed_b, dpts));
}
int lush_mlp_bwd_weights(int net, int planes_f, int planes_b, int R, int S, const lush_mlp_params* prm, const float* draw,
                         const void* stash, void* dstash, const lush_mlp_grads* g, int variant, lush_stream_t stream) {
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw, stash, dstash, variant, stream).weights(g));
}

int lush_mlp_bwd_chain_live(int net, int planes_f, int planes_b, const float* rays, const float* z, int R, int S,
                            const void* packed_b, const lush_mlp_params* prm, const float* draw_c, const void* stash, void* dstash,
                            float* dpts, const int* live_idx, const int* live_cnt, int variant, lush_stream_t stream) {
    if (!live_idx || !live_cnt) return set_error("lush_mlp_bwd_chain_live: live_idx and live_cnt are required");
    // (the loss scale is taken over all R*S rows of draw_c: lush_live_compact zeroed the rows behind the list)
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw_c, stash, dstash, variant, stream).chain(rays, z, packed_b, dpts).live(live_idx, live_cnt));
}
int lush_mlp_bwd_weights_live(int net, int planes_f, int planes_b, int R, int S, const lush_mlp_params* prm, const float* draw_c,
                              const void* stash, void* dstash, const lush_mlp_grads* g, const int* live_cnt, int variant,
                              lush_stream_t stream) {
    if (!live_cnt) return set_error("lush_mlp_bwd_weights_live: live_cnt is required");
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw_c, stash, dstash, variant, stream).weights(g).live(nullptr, live_cnt));
}

// The job table and the plan of the grouped weight-gradient launch that a backward over P points would make on a device of n_cu
// CUs, with dummy base addresses: no device, no HIP call (tests/test_cpu_host.py pins the plan with it).
int lush_debug_dw_plan(int net, int planes_f, int planes_b, long long P, int variant, int live, int n_cu, long long* o) {
    if (!o || n_cu < 1 || P < 1 || P >= (1LL << 27)) return set_error("lush_debug_dw_plan: an output array, n_cu >= 1 and 1 .. 2^27 - 1 points");
    static char dummy[64];                  // addresses that are never followed
    float* const df = (float*)dummy;
    lush_mlp_params prm;
    lush_mlp_grads g;
    for (int l = 0; l < 8; ++l) { prm.w[l] = prm.b[l] = df; g.w[l] = g.b[l] = df; }
    prm.w_feat = prm.b_feat = prm.w_alpha = prm.b_alpha = prm.w_views = prm.b_views = prm.w_rgb = prm.b_rgb = df;
    g.w_feat = g.b_feat = g.w_alpha = g.b_alpha = g.w_views = g.b_views = g.w_rgb = g.b_rgb = df;
    BwdRequest q = bwd_pass(net, planes_f, planes_b, (int)P, 1, &prm, df, dummy, dummy, variant, nullptr).weights(&g);
    if (live) q.live(nullptr, (const int*)dummy);
    BwdCtx c;
    int rc = bwd_context(q, c);
    if (rc) return rc;
    if (c.planes_b > 2) return set_error("lush_debug_dw_plan: three planes take one launch per layer, not the grouped launch");
    DwGroup G{};
    FeatFactorArgs F{};
    rc = dw_job_table(q, c, G, F);
    if (rc) return rc;
    const DwPlan plan = plan_dw_group(G, c.L.Ppad, live != 0, variant, n_cu);
    for (int i = 0; i < 80; ++i) o[i] = -1;
    o[0] = G.n; o[1] = G.per_job; o[2] = G.Ppad; o[3] = G.pts_per_split; o[4] = plan.grid_x; o[5] = plan.grid_y; o[6] = plan.use_cursor ? 1 : 0;
    for (int i = 0; i < G.n; ++i) {
        const DwJob& j = G.j[i];
        long long* w = o + 7 + 6 * i;
        w[0] = j.n_out; w[1] = j.k_in; w[2] = j.k2_in; w[3] = j.pe_mode; w[4] = j.pps; w[5] = G.first[i];
    }
    o[79] = G.first[G.n];
    return 0;
}

}  // extern "C"

// ---- for lush_march_bwd (lush_march_abi.hip), whose compositing backward has already prepared the dstash header ----
namespace lush {
int mlp_bwd_chain_prepared(int net, int planes_f, int planes_b, const float* rays, const float* z, int R, int S,
                           const void* packed_b, const lush_mlp_params* prm, const float* draw, const void* stash,
                           void* dstash, float* dpts, int variant, hipStream_t stream, const int* live_idx, const int* live_cnt) {
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw, stash, dstash, variant, stream).chain(rays, z, packed_b, dpts).live(live_idx, live_cnt).prepared());
}
int mlp_bwd_weights_prepared(int net, int planes_f, int planes_b, int R, int S, const lush_mlp_params* prm, const float* draw,
                             const void* stash, void* dstash, const lush_mlp_grads* g, int variant, hipStream_t stream, const int* live_cnt) {
    return mlp_bwd(bwd_pass(net, planes_f, planes_b, R, S, prm, draw, stash, dstash, variant, stream).weights(g).live(nullptr, live_cnt).prepared());
}
bool mlp_live_kernels(int net, int planes_f, int planes_b, int variant) { return live_kernels(net, planes_f, planes_b, variant); }
// where the header of a dstash holds {scale, 1/scale, work, work} and what the weight-gradient launch needs zero behind them
bool mlp_dstash_header(int net, int planes_b, long long P, void* dstash, float** scale4, float** zero_buf, long long* zero_n) {
    NetInfo n;
    if (!net_info(net, n) || !dstash) return false;
    const int ns = planes_b == PLANES_F16 ? 1 : planes_b;
    const DStashLayout D = dstash_layout(n, ns, P);
    *scale4 = planes_b == PLANES_F16 ? (float*)((char*)dstash + D.scale) : nullptr;
    const ZeroRange zr = ns <= 2 ? dstash_zero_range(D, n, dstash) : ZeroRange{nullptr, 0};
    *zero_buf = zr.p;
    *zero_n = zr.n;
    return true;
}
}  // namespace lush
