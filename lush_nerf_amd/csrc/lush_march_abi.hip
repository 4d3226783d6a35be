// lush-march: ONE C-ABI call per ray march: lush_march_fwd / lush_march_bwd are
// NeRFAll.render_rays_nonoise (models/lushnerf.py:481-583) and its autograd backward, composed on the host from the
// kernels behind the piecewise entry points -- z grid + jitter, weight packing, coarse MLP, compositing, sample_pdf +
// merge, fine MLP, compositing -- enqueued on the caller's stream, working out of ONE caller-provided workspace whose
// size is queried first (lush_march_workspace_bytes).  No allocation, no synchronisation, no state between calls: what
// the backward needs (z, raw, weights, the packed weights, the activation stashes) stays in the workspace.
#include "lush_common.h"
#include "lush_host.h"
#include "../../include/lush_march.h"
#include "../../include/lush_live_fwd.h"
#include "../../include/lush_live_coarse.h"

using namespace lush;

namespace {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int nplanes(int c) { return c == PLANES_F16 ? 1 : c; }
// what the forward keeps for the backward (ops.stash_code): an fp16 forward stashes its single fp16 plane, otherwise the
// first min(forward planes, backward planes) bf16 planes
inline int stash_code(int pf, int pb) { return pb == 0 ? 0 : (pf == PLANES_F16 ? PLANES_F16 : (pf < nplanes(pb) ? pf : nplanes(pb))); }

// One MLP evaluation of the march (the coarse pass, the fine pass) as this configuration runs it: every constant fact of it, decided
// in layout() and nowhere else; the forward, the backward and lush_march_view run from this record.  Offsets are into the workspace.
struct Pass {
    int S;                           // samples per ray
    size_t z, w, raw;                // depths, compositing weights, raw rows
    size_t pk, pkb;                  // the forward's fragments when the caller packed none; where the backward's live or are packed (= pk when the plane codes agree)
    size_t stash, stash_bytes;
    size_t idx, ray_start;           // live-point backward (round 5): the list and the per-ray ranges this pass works on
    bool trunk;                      // its forward runs in the trunk form and leaves its list, per-ray ranges and live stash,
    int fwd_word;                    // the list's length in this word of the count block
    int counts_word;                 // first word of its {live points, points} pair of LUSH_VIEW_LIVE_COUNTS
    int fault_shift;                 // the coarse pass ahead of a fine one reports numerical faults under LUSH_FAULT_COARSE_SHIFT
};

struct Layout {
    Pass coarse, fine;               // (fine: N_importance > 0)
    bool two;                        // a fine pass follows the coarse one, whose results are then rgb0 ..
    bool live;                       // the backward re-runs the forward on the live points (the forward call keeps no stash)
    size_t zs, total;                // z_samples of lush_sample_merge; the size of the workspace
    size_t draw, dstash, dpts;       // backward scratch, shared by the passes (they run one after the other)
    size_t draw_c, live_cnt, live_aux;      // live-point backward: the list's d_raw rows, the 256-byte count block, scan scratch
    const Pass& final_pass() const { return two ? fine : coarse; }
};

// The march of every one- / two-plane mode (the 64-points-per-wave kernels of (h,h), the 128-point chain kernels of the bf16-plane
// modes) keeps NO stash in its forward: the backward lists the points whose d_raw row is non-zero, re-runs the forward with the stash
// on that list and chains / forms the weight gradients on it (include/lush_march.h "Live points").  LUSH_VARIANT_DENSE_BWD keeps the
// rounds 1-4 form.
inline bool live_mode(const lush_march_cfg* c) {
    return c->planes_bwd != 0 && !(c->variant & LUSH_VARIANT_DENSE_BWD) &&
           mlp_live_kernels(0, c->planes_fwd, c->planes_bwd, c->variant & LUSH_VARIANT_KERNEL_BITS & ~LUSH_VARIANT_DENSE_BWD);
}

// The final pass's forward runs trunk-only over all the points and in full, with the stash, on the points of non-zero alpha
// (include/lush_live_fwd.h): the live-point march whose forward is the product's 64-points-per-wave fp16 kernel.  Asked by
// layout() for Pass::trunk and, through lush_march_trunk_form, by the Python side -- nobody restates it.
inline bool trunk_form(const lush_march_cfg* c) {
    return live_mode(c) && c->planes_fwd == PLANES_F16 && !(c->variant & (LUSH_VARIANT_FWD_HALF | LUSH_VARIANT_FWD_512 | LUSH_VARIANT_PE_ROWS));
}

// The coarse pass of a march with a fine pass in the same form (include/lush_live_coarse.h): asked for by a bit of the word, since
// the coarse stash must then survive the fine pass and takes a region of its own.
inline bool coarse_trunk_form(const lush_march_cfg* c) {
    return (c->variant & LUSH_MARCH_COARSE_TRUNK) && c->N_importance > 0 && trunk_form(c);
}

bool layout(const lush_march_cfg* c, Layout& L) {
    if (!c || c->R <= 0 || c->N_samples < 2 || c->N_importance < 0) return false;
    const long long R = c->R, S = c->N_samples, Ni = c->N_importance, Sf = S + Ni;
    // (every MLP launch and lush_live_compact take at most 2^27 - 1 points: refused HERE, not by the first launch that meets them --
    // round 5's layout sized a workspace for such a march and its backward then failed half way)
    if (R * Sf >= (1LL << 27)) return false;
    const int pf = c->planes_fwd, pb = c->planes_bwd, sc = stash_code(pf, pb);
    const size_t pk_f = lush_mlp_packed_bytes(0, pf), pk_b = pb ? lush_mlp_packed_bytes(0, pb) : 0;
    if (pk_f == 0 || (pb && pk_b == 0)) return false;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al256(bytes); return o; };
    L = Layout{};
    L.two = Ni > 0; L.live = pb != 0 && live_mode(c);
    Pass &C = L.coarse, &F = L.fine;
    // The coarse pass.  The only one, it is the final pass: the final pass's form, count word and LIVE_COUNTS pair.  Ahead of a fine
    // one it runs in the trunk form where the word asks for it, with a count word of its own, and reports to the second pair.
    C.S = (int)S; C.trunk = L.two ? coarse_trunk_form(c) : trunk_form(c);
    C.fwd_word = L.two ? LUSH_LIVE_COARSE_LIST_COUNT_WORD : LUSH_LIVE_LIST_COUNT_WORD;
    C.counts_word = L.two ? 2 : 0; C.fault_shift = L.two ? LUSH_FAULT_COARSE_SHIFT : 0;
    C.z = take(R * S * 4); C.w = take(R * S * 4); C.raw = take(R * S * 16); C.pk = take(pk_f);
    C.stash_bytes = lush_mlp_stash_bytes(0, pf, sc, R * S);
    // Live-point march with a fine pass: ONE stash region for both passes.  Its forward keeps no stash (the region is the
    // inference kernels' scratch), its backward re-runs the forward with the stash pass by pass, fine first, and a pass is done with
    // its stash before the next one starts: the coarse pass's region is the head of the fine pass's (-4.4 KB per coarse point of
    // workspace: 5.8 GB at BASELINE config 2).
    // The coarse trunk form is the exception: its forward writes the live coarse rows' stash, which the backward's coarse pass reads
    // after the fine pass has come and gone.
    const bool coarse_own = L.two && C.trunk, share_stash = L.live && L.two && !coarse_own;
    if (!share_stash) C.stash = take(C.stash_bytes);
    if (L.two) {
        F.S = (int)Sf; F.trunk = trunk_form(c); F.fwd_word = LUSH_LIVE_LIST_COUNT_WORD;
        F.z = take(R * Sf * 4); L.zs = take(R * Ni * 4); F.w = take(R * Sf * 4); F.raw = take(R * Sf * 16);
        F.pk = c->same_net ? C.pk : take(pk_f);
        F.stash_bytes = lush_mlp_stash_bytes(0, pf, sc, R * Sf); F.stash = take(F.stash_bytes);
        if (share_stash) C.stash = F.stash;
    }
    if (pb) {
        const long long Pmax = R * Sf;
        // fragments of the backward's plane code: the forward's copy when the codes agree, else a region of their own, one per net
        C.pkb = pb == pf ? C.pk : take(pk_b);
        if (L.two) F.pkb = pb == pf ? F.pk : (c->same_net ? C.pkb : take(pk_b));
        L.draw = take(Pmax * 16); L.dstash = take(lush_mlp_dstash_bytes(0, pb, Pmax)); L.dpts = take(Pmax * 32);
        if (L.live) {
            // one list and one set of per-ray ranges serve both passes, except in the coarse trunk form, whose coarse pass has its own
            F.idx = take(Pmax * 4); L.draw_c = take(Pmax * 16);
            F.ray_start = take(((size_t)R + 1) * 4); L.live_cnt = take(256); L.live_aux = take(lush_live_aux_bytes(Pmax));
            C.idx = coarse_own ? take(R * S * 4) : F.idx; C.ray_start = coarse_own ? take(((size_t)R + 1) * 4) : F.ray_start;
        }
    }
    L.total = off;
    return true;
}

// What a call hands one pass: its net's parameters, the caller's fragments of that net, its noise (pass_args), and per direction ...
struct PassArgs {
    const lush_mlp_params* prm;
    const void *pk, *pkb;            // the caller's fragments of the forward's / the backward's plane code (cfg->packed_*), or null
    bool pack;                       // with none from the caller this pass packs them into the workspace (else an earlier pass of the same net has)
    const float* noise;
    float *rgb, *depth, *acc, *density;          // forward: outputs
    const float *g_rgb, *g_depth, *g_acc;        // backward: output gradients
    const lush_mlp_grads* grads;                 //           and the net's gradient buffers
};

PassArgs pass_args(const lush_march_cfg* c, bool fine_net, const lush_mlp_params* prm, const float* noise) {
    PassArgs a{};
    a.prm = prm; a.pk = fine_net ? c->packed_fine : c->packed_coarse;
    // (pb == pf: the forward's fragments serve -- the caller's buffer if it packed, else the workspace copy at Pass::pkb = Pass::pk)
    a.pkb = c->planes_bwd == c->planes_fwd ? a.pk : (fine_net ? c->packed_bwd_fine : c->packed_bwd_coarse);
    a.noise = c->raw_noise_std > 0.f ? noise : nullptr;
    return a;
}

// One lush_march_fwd / lush_march_bwd: what every pass of the call works with, and the passes.  (var: what the launchers see, no
// layout or permission bit; flags: the forward's numerical-fault word; drays: the backward's d(ray batch))
struct Call {
    const lush_march_cfg* cfg; const Layout& L; const float* rays; char* w;
    int pf, pb, var; lush_stream_t st; int* flags; float* drays;
    int fwd_pass(const Pass& P, const PassArgs& a) const;
    int bwd_pass(const Pass& P, const PassArgs& a, bool from_fwd, bool first_pass) const;
};

// One pass of the forward: pack if needed, the MLP in the pass's form, compositing.
int Call::fwd_pass(const Pass& P, const PassArgs& a) const {
    // weights: packed by the caller once per step (cfg->packed_*), or here into the workspace
    const void* pk = a.pk;
    if (!pk) {
        pk = w + P.pk;
        if (a.pack)
            if (int rc = lush_mlp_pack_for(0, pf, a.prm, w + P.pk, var, st)) return rc;
    }
    const int R = cfg->R, sc = stash_code(pf, pb);
    const float* z = (const float*)(w + P.z);
    float* raw = (float*)(w + P.raw);
    if (!P.trunk) {      // (live-point backward: the forward keeps raw, z, weights only)
        if (int rc = lush_mlp_fwd(0, pf, L.live ? 0 : sc, rays, z, R, P.S, pk, a.prm, raw, w + P.stash, var, st)) return rc;
    } else {
        // The trunk form: sigma of every point, the list of the points whose alpha is not zero (into the backward's list regions;
        // its length beside the LIVE_COUNTS words), all of the net WITH the stash on the list, which writes their rows.  A row the
        // list leaves out keeps rgb = 0: finite, and multiplied by a weight of exactly 0.  The coarse pass ahead of a fine one runs
        // the same way in the coarse trunk form (include/lush_live_coarse.h), with its own stash, list and ranges and its own count
        // word; the scan scratch serves one list after the other.
        int *lidx = (int*)(w + P.idx), *ray_start = (int*)(w + P.ray_start), *list_cnt = (int*)(w + L.live_cnt) + P.fwd_word;
        if (int rc = lush_mlp_fwd_trunk(0, pf, rays, z, R, P.S, pk, raw, w + P.stash, var, st)) return rc;
        if (int rc = lush_live_list(raw, z, a.noise, cfg->raw_noise_std, cfg->near_mask, R, P.S, lidx, ray_start, list_cnt, w + L.live_aux, st)) return rc;
        if (int rc = lush_mlp_fwd_live_raw(0, pf, sc, rays, z, R, P.S, pk, w + P.stash, lidx, list_cnt, raw, var, st)) return rc;
    }
    return lush_composite_fwd(raw, z, rays, R, P.S, a.noise, cfg->raw_noise_std, cfg->near_mask, cfg->white_bkgd,
                              a.rgb, a.depth, a.acc, (float*)(w + P.w), a.density, flags, P.fault_shift, st);
}

// One pass of the backward = compositing backward, (re-pack), gradient chain, d(point) -> d(ray), weight gradients, out of the one
// backward scratch.  from_fwd: the pass works on the list, per-ray ranges and stash its forward left (Pass::trunk, and the caller
// vouches for the workspace); first_pass: it writes d(ray) whole.
int Call::bwd_pass(const Pass& P, const PassArgs& a, bool from_fwd, bool first_pass) const {
    const int R = cfg->R, Sp = P.S, sc = stash_code(pf, pb);
    const float* z = (const float*)(w + P.z);
    float *draw = (float*)(w + L.draw), *dpts = (float*)(w + L.dpts);
    char* dstash = w + L.dstash;
    // the compositing backward also leaves the per-workgroup maxima of |d_raw| (in the d(point) array, which the chain only
    // writes afterwards) for the fp16 chain's loss scale, zeroes the weight-gradient scratch and, in the march's first pass,
    // writes d(ray) whole: no pass over d_raw for the scale, no memsets, no zero-fill of drays by the caller
    float *scale4 = nullptr, *zero_buf = nullptr;
    long long zero_n = 0;
    if (!mlp_dstash_header(0, pb, (long long)R * Sp, dstash, &scale4, &zero_buf, &zero_n)) return set_error("lush_march_bwd: bad backward plane code");
    float* block_max = scale4 ? dpts : nullptr;
    if (int rc = lush_composite_bwd((const float*)(w + P.raw), z, rays, R, Sp, a.noise, cfg->raw_noise_std, cfg->near_mask, cfg->white_bkgd,
                                    a.g_rgb, a.g_depth, a.g_acc, draw, drays, block_max, zero_buf, zero_n, first_pass ? 1 : 0, st)) return rc;
    if (scale4)
        if (int rc = lush_loss_scale(block_max, lush_composite_bwd_blocks(R), scale4, st)) return rc;
    // fragments of the backward's plane code: the caller's (cfg->packed_*), else the forward's copy in the workspace when the
    // codes agree, else packed here
    const void* pk = a.pkb;
    if (!pk) {
        pk = w + P.pkb;
        if (a.pack)         // the backward computes with another plane code than the forward: its own fragments
            if (int rc = lush_mlp_pack_for(0, pb, a.prm, w + P.pkb, var, st)) return rc;
    }
    const float* rows = draw;            // over all the points: every d_raw row, no list
    int *lidx = nullptr, *ray_start = nullptr;
    const int* len = nullptr;            // the length of the list the launches below run on
    if (L.live) {
        // the live points of this pass: list, gathered d_raw rows, per-ray ranges (three small launches); the forward once
        // more, WITH the stash, on the list; then chain, d(ray) and weight gradients on `len` points (read on the device)
        lidx = (int*)(w + P.idx); ray_start = (int*)(w + P.ray_start);
        int* lcnt = (int*)(w + L.live_cnt) + P.counts_word;      // {live points, points} of this pass: LUSH_VIEW_LIVE_COUNTS
        float* draw_c = (float*)(w + L.draw_c);
        rows = draw_c;
        if (from_fwd) {
            // the forward's list, per-ray ranges and stash stand: d_raw rows in list order (a listed point may have a zero row:
            // it adds exact zeros), and the count of the non-zero ones for LIVE_COUNTS
            len = (const int*)(w + L.live_cnt) + P.fwd_word;
            if (int rc = lush_live_gather(draw, R, Sp, lidx, len, draw_c, lcnt, st)) return rc;
        } else {
            len = lcnt;
            if (int rc = lush_live_compact(draw, R, Sp, lidx, draw_c, ray_start, lcnt, w + L.live_aux, st)) return rc;
            const void* pk_fwd = a.pk ? a.pk : (const void*)(w + P.pk);      // forward fragments: the caller's buffer or the forward call's copy in the workspace
            if (int rc = lush_mlp_fwd_live(0, pf, sc, rays, z, R, Sp, pk_fwd, a.prm, w + P.stash, lidx, lcnt, var, st)) return rc;
        }
    }
    if (int rc = mlp_bwd_chain_prepared(0, sc, pb, rays, z, R, Sp, pk, a.prm, rows, w + P.stash, dstash, dpts, var, (hipStream_t)st, lidx, len)) return rc;
    if (int rc = L.live ? lush_ray_grad_reduce_live(dpts, z, lidx, ray_start, R, drays, st) : lush_ray_grad_reduce(dpts, z, R, Sp, drays, st)) return rc;
    return mlp_bwd_weights_prepared(0, sc, pb, R, Sp, a.prm, rows, w + P.stash, dstash, a.grads, var, (hipStream_t)st, len);
}

}  // namespace

extern "C" {

size_t lush_march_workspace_bytes(const lush_march_cfg* cfg) {
    Layout L;
    return layout(cfg, L) ? L.total : 0;
}

int lush_march_view(const lush_march_cfg* cfg, int which, size_t* offset, size_t* bytes) {
    Layout L;
    if (!layout(cfg, L) || !offset || !bytes) return set_error("lush_march_view: bad configuration");
    const long long R = cfg->R;
    const Pass& P = L.final_pass();
    switch (which) {
        case LUSH_VIEW_Z: *offset = P.z; *bytes = R * P.S * 4; return 0;
        case LUSH_VIEW_RAW: *offset = P.raw; *bytes = R * P.S * 16; return 0;
        case LUSH_VIEW_WEIGHTS: *offset = P.w; *bytes = R * P.S * 4; return 0;
        case LUSH_VIEW_Z_COARSE: *offset = L.coarse.z; *bytes = R * L.coarse.S * 4; return 0;
        case LUSH_VIEW_STASH_COARSE: *offset = L.coarse.stash; *bytes = L.coarse.stash_bytes; return 0;
        case LUSH_VIEW_STASH_FINE:
            if (!L.two) return set_error("lush_march_view: no fine pass");
            *offset = L.fine.stash; *bytes = L.fine.stash_bytes; return 0;
        case LUSH_VIEW_LIVE_COUNTS:
            if (!L.live) return set_error("lush_march_view: this configuration's backward runs over all the points");
            *offset = L.live_cnt; *bytes = 16; return 0;
        default: return set_error("lush_march_view: unknown view");
    }
}

int lush_march_trunk_form(const lush_march_cfg* cfg) {
    Layout L;
    return layout(cfg, L) && trunk_form(cfg) ? 1 : 0;
}

int lush_march_coarse_trunk_form(const lush_march_cfg* cfg) {
    Layout L;
    return layout(cfg, L) && coarse_trunk_form(cfg) ? 1 : 0;
}

int lush_march_fwd(const lush_march_cfg* cfg, const float* rays, const lush_mlp_params* coarse, const lush_mlp_params* fine,
                   const lush_march_draws* draws, const lush_march_out* out, void* workspace, int* flags, lush_stream_t st) {
    Layout L;
    if (!layout(cfg, L)) return set_error("lush_march_fwd: bad configuration");
    if (!rays || !coarse || !out || !workspace) return set_error("lush_march_fwd: rays, coarse parameters, outputs and workspace are required");
    const bool two = L.two;
    if (two && !cfg->same_net && !fine) return set_error("lush_march_fwd: the fine parameters are required");
    if (!out->rgb || !out->depth || !out->acc || !out->density) return set_error("lush_march_fwd: rgb, depth, acc, density outputs are required");
    if (two && (!out->rgb0 || !out->depth0 || !out->acc0 || !out->density0 || !out->z_std)) return set_error("lush_march_fwd: the coarse outputs and z_std are required when N_importance > 0");
    char* w = (char*)workspace;
    const Call m{cfg, L, rays, w, cfg->planes_fwd, cfg->planes_bwd, cfg->variant & LUSH_VARIANT_KERNEL_BITS, st, flags, nullptr};
    const bool jitter = draws && cfg->perturb > 0.f;
    PassArgs ac = pass_args(cfg, false, coarse, draws ? draws->noise_c : nullptr);
    PassArgs af = pass_args(cfg, !cfg->same_net, cfg->same_net ? coarse : fine, draws ? draws->noise_f : nullptr);
    ac.pack = true; af.pack = !cfg->same_net;       // (one net: the coarse pass has packed it)
    // the coarse pass's results are rgb0 .. when a fine pass follows, else the final ones
    ac.rgb = two ? out->rgb0 : out->rgb; ac.depth = two ? out->depth0 : out->depth; ac.acc = two ? out->acc0 : out->acc; ac.density = two ? out->density0 : out->density;
    af.rgb = out->rgb; af.depth = out->depth; af.acc = out->acc; af.density = out->density;
    float* zc = (float*)(w + L.coarse.z);
    if (int rc = lush_zgrid(rays, cfg->R, L.coarse.S, cfg->lindisp, jitter ? draws->t_rand : nullptr, zc, st)) return rc;
    const int rc = m.fwd_pass(L.coarse, ac);
    if (rc || !two) return rc;
    if (int rm = lush_sample_merge(zc, (const float*)(w + L.coarse.w), cfg->R, L.coarse.S, cfg->N_importance, jitter ? draws->u : nullptr,
                                   (float*)(w + L.fine.z), (float*)(w + L.zs), out->z_std, flags, st)) return rm;
    return m.fwd_pass(L.fine, af);
}

int lush_march_bwd(const lush_march_cfg* cfg, const float* rays, const lush_mlp_params* coarse, const lush_mlp_params* fine,
                   const lush_march_draws* draws, const lush_march_gout* g, void* workspace, const lush_mlp_grads* g_coarse,
                   const lush_mlp_grads* g_fine, float* drays, lush_stream_t st) {
    Layout L;
    if (!layout(cfg, L)) return set_error("lush_march_bwd: bad configuration");
    if (cfg->planes_bwd == 0) return set_error("lush_march_bwd: the forward ran as inference (planes_bwd = 0): nothing was kept");
    if (!rays || !coarse || !g || !workspace || !drays) return set_error("lush_march_bwd: rays, parameters, output gradients, workspace and drays are required");
    const bool two = L.two;
    const int pf = cfg->planes_fwd, pb = cfg->planes_bwd;
    const Call m{cfg, L, rays, (char*)workspace, pf, pb, cfg->variant & LUSH_VARIANT_KERNEL_BITS, st, nullptr, drays};
    PassArgs ac = pass_args(cfg, false, coarse, draws ? draws->noise_c : nullptr);
    PassArgs af = pass_args(cfg, !cfg->same_net, cfg->same_net ? coarse : fine, draws ? draws->noise_f : nullptr);
    ac.grads = g_coarse; af.grads = cfg->same_net ? g_coarse : g_fine;
    af.g_rgb = g->rgb; af.g_depth = g->depth; af.g_acc = g->acc;
    ac.g_rgb = two ? g->rgb0 : g->rgb; ac.g_depth = two ? g->depth0 : g->depth; ac.g_acc = two ? g->acc0 : g->acc;
    const bool any_main = g->rgb || g->depth || g->acc, any_c = ac.g_rgb || ac.g_depth || ac.g_acc;
    if ((two && any_main && !af.grads) || (any_c && !g_coarse))
        return set_error("lush_march_bwd: gradient buffers of a pass that received output gradients are required");
    // The caller vouches that the workspace is as the lush_march_fwd of this configuration left it: a pass whose forward ran in the
    // trunk form then works on the forward's list and stash (include/lush_live_fwd.h): the final pass, and the coarse pass ahead of it
    // in the coarse trunk form alone.  Without the bit every pass lists its live points and re-runs the forward on them, which is
    // correct after any forward.
    const bool kept = (cfg->variant & LUSH_MARCH_FWD_LIST_KEPT) && L.final_pass().trunk, kept_c = kept && L.coarse.trunk;
    // The fine pass first, then the coarse one (which does not depend on it: z_samples are detached, models/lushnerf.py:546), all
    // on the caller's stream out of one backward scratch.  (Round 3 ran the fine pass's weight gradients on a second stream beside
    // the coarse chain, each on part of the chip: both kernels slowed down side by side -- HBM and power are shared -- and the step
    // gained 0.4 ms on one box and lost 0.3 on two others, the driver's among them; removed in round 4)
    bool first_pass = true, packed_b_c = false;
    if (two && any_main) {
        af.pack = pb != pf;
        if (int rc = m.bwd_pass(L.fine, af, kept, first_pass)) return rc;
        first_pass = false;
        packed_b_c = cfg->same_net && pb != pf;     // the shared net's backward fragments are packed now
    }
    if (!any_c) return 0;
    ac.pack = pb != pf && !packed_b_c;
    return m.bwd_pass(L.coarse, ac, kept_c, first_pass);
}

}  // extern "C"
