/* lush-march C ABI, third contract header: the training march whose final pass computes colour on live points only.
 *
 * Same library (liblush_march.so), same conventions as lush_march.h, which this header includes for its types.
 * lush_march.h is ABI version 10 and stays as it is; what is declared here is read into a table of its own
 * (lush_nerf_amd/lib.py: EXPORTS_LIVE_FWD).
 *
 * THE FORM.  A sample whose density pre-activation (+ noise) fails the clamp of raw2outputs, or which near_mask hides, has
 * alpha = 0 and weight = 0: its colour is multiplied by an exact zero in the forward and receives an exactly zero gradient.
 * In the headline mode (forward plane code 17 on the 64-points-per-wave kernel, live-point backward) lush_march_fwd
 * therefore runs the FINAL pass -- the fine pass when N_importance > 0, else the only pass -- as
 *     trunk-only forward over all the points (layers 0..7 + alpha head: raw = (0, 0, 0, sigma))
 *     -> the list of the points the compositing gives a non-zero alpha (lush_live_list)
 *     -> the full forward WITH the stash on that list, which writes their raw rows (lush_mlp_fwd_live_raw)
 *     -> lush_composite_fwd as before.
 * The rendered outputs are bit-identical to the other forms'.  NOTE for `retraw`: the raw rows (LUSH_VIEW_RAW) of a training
 * march in this form carry rgb = 0 at the samples of zero weight; sigma is complete.  lush_march_trunk_form(cfg) says whether a
 * configuration runs in this form (inference, LUSH_VARIANT_DENSE_BWD, the older-kernel variants and every other precision
 * mode do not).
 *
 * The backward needs nothing new: where d_raw can be non-zero, raw is complete, so lush_march_bwd WITHOUT the bit below lists
 * the live points and re-runs the forward on them as it always did.  A caller who knows that NOTHING has touched the
 * workspace since the lush_march_fwd of the same configuration may set LUSH_MARCH_FWD_LIST_KEPT in cfg->variant of
 * lush_march_bwd: the final pass then works on the forward's list and stash (its d_raw rows gathered in list order) and the
 * second evaluation of the live points is saved.  The bit is valid for ONE lush_march_bwd call after a lush_march_fwd: the
 * coarse pass of that call re-uses the stash region.  It is ignored where the form does not apply. */
#ifndef LUSH_LIVE_FWD_H
#define LUSH_LIVE_FWD_H
#include "lush_march.h"

#define LUSH_MARCH_FWD_LIST_KEPT 65536    /* outside LUSH_VARIANT_KERNEL_BITS: selects no kernel */
#define LUSH_LIVE_LIST_COUNT_WORD 8       /* int index in the 256-byte count block (LUSH_VIEW_LIVE_COUNTS offset): {length of the forward's list, points} */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when lush_march_fwd / lush_march_bwd run this configuration in the form above, else 0. */
int lush_march_trunk_form(const lush_march_cfg* cfg);

/* The pieces, for callers who compose a march themselves (arguments as their lush_march.h counterparts).
 * lush_mlp_fwd_trunk: net 0, planes = LUSH_PLANES_F16, no older-kernel variant; raw [R*S][4] = (0, 0, 0, sigma) with sigma
 *   bit-identical to lush_mlp_fwd's; `workspace` as lush_mlp_fwd's stash argument with stash_planes = 0.
 * lush_live_list: point p = r*S + j is listed iff j == S-1, or raw[p][3] + noise[r*(S-1)+j]*noise_std > 0 and near_mask does
 *   not hide it (near_mask < 0 or z[p+1] > near_mask) -- the condition of lush_composite_fwd for alpha != 0.  In grid order:
 *   live_idx [R*S] (the first cnt[0] entries), ray_start [R+1], cnt = {length, R*S}; aux of lush_live_aux_bytes(R*S).
 * lush_mlp_fwd_live_raw: lush_mlp_fwd_live which also writes the i-th point's row to raw[live_idx[i]] (raw NULL: no store).
 * lush_live_gather: draw_c[i] = draw[live_idx[i]] for i < list_cnt[0], zero rows behind them up to R*S;
 *   cnt = {rows of the list that are non-zero, R*S}. */
int lush_mlp_fwd_trunk(int net, int planes, const float* rays, const float* z, int R, int S, const void* packed, float* raw,
                       void* workspace, int variant, lush_stream_t stream);
int lush_live_list(const float* raw, const float* z, const float* noise, float noise_std, float near_mask, int R, int S,
                   int* live_idx, int* ray_start, int* cnt, void* aux, lush_stream_t stream);
int lush_mlp_fwd_live_raw(int net, int planes, int stash_planes, const float* rays, const float* z, int R, int S,
                          const void* packed, void* stash, const int* live_idx, const int* live_cnt, float* raw, int variant,
                          lush_stream_t stream);
int lush_live_gather(const float* draw, int R, int S, const int* live_idx, const int* list_cnt, float* draw_c, int* cnt,
                     lush_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
