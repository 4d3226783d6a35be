/* lush-march C ABI, fourth contract header: the training march whose COARSE pass, too, computes colour on live points only.
 *
 * Same library (liblush_march.so), same conventions as lush_march.h, which this header includes for its types; lush_march.h
 * (ABI version 10), lush_subframe.h and lush_live_fwd.h stay as they are.  What is declared here is read into a table of its own
 * (lush_nerf_amd/lib.py: EXPORTS_LIVE_COARSE).
 *
 * THE FORM.  lush_live_fwd.h runs the FINAL pass of the headline mode's training march trunk-only over all the points and in
 * full, with the stash, on the points of non-zero alpha.  The coarse pass of a march with N_importance > 0 kept the full forward
 * over all its points and a second, stashing forward on its live points inside lush_march_bwd, because its stash shared the
 * fine pass's region and could not survive the fine pass.  With LUSH_MARCH_COARSE_TRUNK in cfg->variant of
 * lush_march_workspace_bytes, lush_march_view, lush_march_fwd and lush_march_bwd -- the SAME word in all four, they lay the
 * workspace out from it -- the coarse pass gets a stash region, a list and per-ray ranges of its own
 * (lush_mlp_stash_bytes(0, planes_fwd, stash planes, R * N_samples) + 4 * R * N_samples + 4 * (R + 1) bytes, each rounded up to
 * 256: 4.9 KB per coarse point) and lush_march_fwd runs it as the final pass runs:
 *     lush_mlp_fwd_trunk over all R * N_samples points -> lush_live_list (noise_c, raw_noise_std, near_mask)
 *     -> lush_mlp_fwd_live_raw WITH the stash on that list -> lush_composite_fwd, lush_sample_merge as before.
 * The rendered outputs (rgb0 .. z_std and everything of the fine pass) are bit-identical to the other forms'.  NOTE for `retraw`:
 * the COARSE raw rows of a training march in this form carry rgb = 0 at the samples of zero weight, as the final pass's do;
 * sigma is complete.
 *
 * lush_march_bwd with the bit and LUSH_MARCH_FWD_LIST_KEPT works on the forward's list and stash in the coarse pass as well
 * (its d_raw rows gathered in list order: no second evaluation of the live coarse points); LUSH_VIEW_LIVE_COUNTS carries the
 * same words as ever.  Without LUSH_MARCH_FWD_LIST_KEPT the coarse pass lists by d_raw and re-runs the live forward, into the
 * coarse region, which is correct after any forward.  The bit is ignored -- offsets, sizes, launches all as without it -- where
 * lush_march_coarse_trunk_form says 0. */
#ifndef LUSH_LIVE_COARSE_H
#define LUSH_LIVE_COARSE_H
#include "lush_march.h"

#define LUSH_MARCH_COARSE_TRUNK 131072         /* outside LUSH_VARIANT_KERNEL_BITS, not LUSH_MARCH_FWD_LIST_KEPT: selects no kernel */
#define LUSH_LIVE_COARSE_LIST_COUNT_WORD 12    /* int index in the 256-byte count block (LUSH_VIEW_LIVE_COUNTS offset): {length of the coarse forward's list, points} */

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when cfg->variant carries LUSH_MARCH_COARSE_TRUNK, lush_march_trunk_form(cfg) holds and N_importance > 0, else 0. */
int lush_march_coarse_trunk_form(const lush_march_cfg* cfg);

#ifdef __cplusplus
}
#endif
#endif
