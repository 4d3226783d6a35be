/* lush-march C ABI, second contract header: the sharp sub-frames of one training view.
 *
 * Same library (liblush_march.so), same conventions as lush_march.h, which this header includes for lush_stream_t and
 * the calling convention.  lush_march.h is ABI version 10 and stays as it is; what is declared here is read into a
 * table of its own (lush_nerf_amd/lib.py: EXPORTS_SUBFRAME).
 */
#ifndef LUSH_SUBFRAME_H
#define LUSH_SUBFRAME_H
#include "lush_march.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ray batch of NeRFAll.render_warped_path (models/lushnerf.py:898-947) for ONE pose in ONE kernel: get_rays for every
 * pixel (:917; utils/run_lushnerf_helpers.py:517-528, pixel centres), the blur kernel's SE(3) warp of the view image_idx[0]
 * (:921-925; models/lushnerf.py:75-98, utils/rigid_warping.py:20-140) and the head of render_train_scene (:929 -> :772-795;
 * ndc_rays helpers:542-562).  The reference orders the rows ray-major and permutes the rendered images afterwards (:932-933);
 * here the rows are SUB-FRAME-MAJOR, so what the march returns is [M+1][H][W] as it stands:
 *   c2w [3][4]; fx, fy, kx, ky = K[0][0], K[1][1], K[0][2], K[1][2]; image_idx [1] int64 ON THE DEVICE (read by the kernel,
 *   clamped to 0 .. num_img-1); acts [num_img][LUSH_RBK_ACT_STRIDE] of lush_rbk_mlp_fwd; ndc, cx, cy, near, far as
 *   lush_pack_rays_fwd  ->  batch [(M+1)*H*W][11], row m*H*W + y*W + x = sub-frame m (0: the un-warped ray) of pixel (x, y);
 *   centre_rays [M+1][3][2] (may be NULL): the warped rays of pixel (W/2, H/2) before the head, what :926 keeps.
 * LIMIT: 1 <= M <= 4, H*W*(M+1) < 2^31. */
int lush_warp_image_fwd(const float* c2w, int H, int W, float fx, float fy, float kx, float ky, const int64_t* image_idx,
                        int num_img, int M, const float* acts, int ndc, float cx, float cy, float near, float far,
                        float* batch, float* centre_rays, lush_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
