// lush-march: the ray prologue + its C ABI -- rays from poses and pixels (get_rays / get_rays_np, utils/run_lushnerf_helpers.py:517-539;
// Render_Aligned_Pixel's gather, models/lushnerf.py:958-985) and the batch rows of rays the caller holds (lush_rays.h).
#include "lush_common.h"
#include "lush_host.h"
#include "lush_rays.h"
#include "../../include/lush_march.h"

namespace lush {

__global__ void pack_rays_fwd_kernel(const float* __restrict__ rays, int N, int ndc, float cx, float cy, float near,
                                     float far, float* __restrict__ batch) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* r = rays + (long long)n * 6;          // [3][2]: r[2*i] = o_i, r[2*i+1] = d_i
    const float o[3] = {r[0], r[2], r[4]}, d[3] = {r[1], r[3], r[5]};
    pack_one(o, d, ndc, cx, cy, near, far, batch + (long long)n * 11);
}

__global__ void pack_rays_bwd_kernel(const float* __restrict__ rays, int N, int ndc, float cx, float cy,
                                     const float* __restrict__ dbatch, float* __restrict__ drays) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* r = rays + (long long)n * 6;
    const float o[3] = {r[0], r[2], r[4]}, d[3] = {r[1], r[3], r[5]};
    float go[3], gd[3];
    pack_one_bwd(o, d, ndc, cx, cy, dbatch + (long long)n * 11, go, gd);
    float* out = drays + (long long)n * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) { out[2 * i] = go[i]; out[2 * i + 1] = gd[i]; }
}

// ------------------------------------------------------- device-side ray table
// get_rays / get_rays_np (utils/run_lushnerf_helpers.py:517-539) evaluated for N (view, pixel) pairs:
// dirs = [(i + 0.5 - cx)/fx, -(j + 0.5 - cy)/fy, -1], rays_d = R dirs (sum over the last axis of
// dirs[None,:] * c2w[:3,:3]), rays_o = c2w[:3,3].  Replaces the pre-materialised [N_img*H*W, 2, 3] table
// and its per-epoch host permutation (run_lushnerf.py:561-589, 610-614).
__global__ void gen_rays_kernel(const float* __restrict__ c2w, const int64_t* __restrict__ view,
                                const int64_t* __restrict__ px, const int64_t* __restrict__ py, int N, float fx,
                                float fy, float cx, float cy, float* __restrict__ rays) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* M = c2w + view[n] * 12;                       // [3][4] row-major
    const float d0 = ((float)px[n] + (0.5f - cx)) / fx;
    const float d1 = -((float)py[n] + (0.5f - cy)) / fy;
    const float d2 = -1.f;
    float* o = rays + (long long)n * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[2 * i] = M[i * 4 + 3];
        o[2 * i + 1] = (d0 * M[i * 4 + 0] + d1 * M[i * 4 + 1]) + d2 * M[i * 4 + 2];
    }
}

// All H*W pixels of ONE pose in row-major pixel order (the eval path's get_rays, helpers:517-528).
__global__ void gen_rays_image_kernel(const float* __restrict__ c2w, int H, int W, float fx, float fy, float cx,
                                      float cy, float* __restrict__ rays) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= H * W) return;
    const int px = n % W, py = n / W;
    const float d0 = ((float)px + (0.5f - cx)) / fx;
    const float d1 = -((float)py + (0.5f - cy)) / fy;
    const float d2 = -1.f;
    float* o = rays + (long long)n * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[2 * i] = c2w[i * 4 + 3];
        o[2 * i + 1] = (d0 * c2w[i * 4 + 0] + d1 * c2w[i * 4 + 1]) + d2 * c2w[i * 4 + 2];
    }
}

// ------------------------------------------------- consistency branch
// Render_Aligned_Pixel's gather (models/lushnerf.py:958-985): for pose v and sample s the matched
// pixel is (x, y) = align[v][samples[s]][2:4].long(), clamped to the image; its ray is row
// [y][x] of get_rays(H, W, K, c2w[v]).  One thread per (v, s).
__global__ void align_rays_kernel(const float* __restrict__ c2w, const float* __restrict__ align,
                                  const void* __restrict__ cert, int cert_is_u8, const int64_t* __restrict__ samples,
                                  int V, int ns, long long HW, int H, int W, float fx, float fy, float cx, float cy,
                                  float* __restrict__ rays, float* __restrict__ cert_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= V * ns) return;
    const int v = t / ns, s = t % ns;
    long long pix = samples[s];
    pix = pix < 0 ? 0 : (pix >= HW ? HW - 1 : pix);     // memory safety only: the reference would raise an IndexError
    const float* a = align + ((long long)v * HW + pix) * 4;
    long long x = (long long)a[2], y = (long long)a[3];          // .long(): truncation toward zero
    x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
    y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
    const float* M = c2w + (long long)v * 12;
    const float d0 = ((float)x + (0.5f - cx)) / fx;
    const float d1 = -((float)y + (0.5f - cy)) / fy;
    const float d2 = -1.f;
    float* o = rays + (long long)t * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o[2 * i] = M[i * 4 + 3];
        o[2 * i + 1] = (d0 * M[i * 4 + 0] + d1 * M[i * 4 + 1]) + d2 * M[i * 4 + 2];
    }
    const long long ci = (long long)v * HW + pix;
    cert_out[t] = cert_is_u8 ? (float)(reinterpret_cast<const uint8_t*>(cert)[ci] != 0) : reinterpret_cast<const float*>(cert)[ci];
}

}  // namespace lush

using namespace lush;

extern "C" {

int lush_pack_rays_fwd(const float* rays, int N, int ndc, float cx, float cy, float near, float far, float* batch,
                       lush_stream_t st) {
    return launch(pack_rays_fwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, rays, N, ndc, cx, cy, near, far, batch);
}
int lush_pack_rays_bwd(const float* rays, int N, int ndc, float cx, float cy, const float* dbatch, float* drays,
                       lush_stream_t st) {
    return launch(pack_rays_bwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, rays, N, ndc, cx, cy, dbatch, drays);
}

int lush_gen_rays(const float* c2w, const int64_t* view, const int64_t* px, const int64_t* py, int N, float fx,
                  float fy, float cx, float cy, float* rays, lush_stream_t st) {
    if (N <= 0) return 0;
    return launch(gen_rays_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, c2w, view, px, py, N, fx, fy, cx, cy, rays);
}

int lush_gen_rays_image(const float* c2w, int H, int W, float fx, float fy, float cx, float cy, float* rays,
                        lush_stream_t st) {
    if (H <= 0 || W <= 0) return set_error("lush_gen_rays_image: empty image");
    return launch(gen_rays_image_kernel, dim3(cdiv((long long)H * W, 256)), dim3(256), 0, st, c2w, H, W, fx, fy, cx, cy, rays);
}

int lush_align_rays(const float* c2w, const float* align, const void* cert, int cert_is_u8, const int64_t* samples,
                    int V, int ns, long long HW, int H, int W, float fx, float fy, float cx, float cy, float* rays,
                    float* cert_out, lush_stream_t st) {
    if (V <= 0 || ns <= 0) return set_error("lush_align_rays: empty");
    if (HW <= 0) return set_error("lush_align_rays: empty match table");
    return launch(align_rays_kernel, dim3(cdiv((long long)V * ns, 128)), dim3(128), 0, st, c2w, align, cert, cert_is_u8,
                  samples, V, ns, HW, H, W, fx, fy, cx, cy, rays, cert_out);
}

}  // extern "C"
