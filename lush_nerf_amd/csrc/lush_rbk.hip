// lush-march: the rigid blurring kernel + its C ABI (Rigid_Blurring_Kernel, models/lushnerf.py:30-116; utils/rigid_warping.py) --
// the SE(3) warp of rays, alone and fused with the batch head (lush_rays.h), forward and backward, and the small MLP that
// produces the motions, resident in LDS.
#include "lush_common.h"
#include "lush_host.h"
#include "lush_rays.h"
#include "../../include/lush_march.h"
#include "../../include/lush_subframe.h"

namespace lush {

// ---------------------------------------------------------------- SE(3) warp
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

struct Se3 { V3 w, nu; float theta, s, c, rn; };   // rn = |r|
__device__ __forceinline__ Se3 se3_setup(V3 r, V3 v) {
    Se3 q;
    q.rn = sqrtf(dot(r, r));
    q.theta = q.rn + 1.0e-10f;
    q.w = (1.f / q.theta) * r;
    q.nu = (1.f / q.theta) * v;
    sincosf(q.theta, &q.s, &q.c);
    return q;
}
// utils/rigid_warping.py:20-45 in closed form: y = R p + t
__device__ __forceinline__ V3 se3_apply(const Se3& q, V3 p) {
    const V3 a = cross(q.w, p), b = cross(q.w, a);
    const V3 e = cross(q.w, q.nu), f = cross(q.w, e);
    return p + q.s * a + (1.f - q.c) * b + q.theta * q.nu + (1.f - q.c) * e + (q.theta - q.s) * f;
}
// reverse mode of se3_apply for one point: adds into gp, and into (gw, gnu, gth, gs, gc)
__device__ __forceinline__ void se3_apply_bwd(const Se3& q, V3 p, V3 gy, V3& gp, V3& gw, V3& gnu, float& gth,
                                              float& gs, float& gc) {
    const V3 a = cross(q.w, p), b = cross(q.w, a);
    const V3 e = cross(q.w, q.nu), f = cross(q.w, e);
    gp = gp + gy;
    gs += dot(gy, a) - dot(gy, f);
    gc += -dot(gy, b) - dot(gy, e);
    gth += dot(gy, q.nu) + dot(gy, f);
    V3 ga = q.s * gy, gb = (1.f - q.c) * gy;
    V3 ge = (1.f - q.c) * gy, gf = (q.theta - q.s) * gy;
    gnu = gnu + q.theta * gy;
    // b = w x a
    gw = gw + cross(a, gb); ga = ga + cross(gb, q.w);
    // a = w x p
    gw = gw + cross(p, ga); gp = gp + cross(ga, q.w);
    // f = w x e
    gw = gw + cross(e, gf); ge = ge + cross(gf, q.w);
    // e = w x nu
    gw = gw + cross(q.nu, ge); gnu = gnu + cross(ge, q.w);
}
// finish: adjoints of (w, nu, theta, s, c) -> (r, v)
__device__ __forceinline__ void se3_finish_bwd(const Se3& q, V3 r, V3 gw, V3 gnu, float gth, float gs, float gc,
                                               V3& gr, V3& gv) {
    gth += gs * q.c - gc * q.s;
    const float it = 1.f / q.theta;
    gth -= it * (dot(gw, q.w) + dot(gnu, q.nu));
    gr = it * gw;
    gv = it * gnu;
    if (q.rn > 0.f) gr = gr + (gth / q.rn) * r;
}

// acts layout per image (LUSH_RBK_ACT_STRIDE floats)
constexpr int RA_E = 0, RA_H0 = 64, RA_HR = 320, RA_HV = 352, RA_HW = 384, RA_WS = 416, RA_R = 424, RA_V = 440,
              RA_WN = 456;

__global__ void rbk_warp_fwd_kernel(const float* __restrict__ rays, const int64_t* __restrict__ idx, int N, int M,
                                    const float* __restrict__ acts, float* __restrict__ new_rays,
                                    float* __restrict__ ccw) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* r6 = rays + (long long)n * 6;
    const V3 o = {r6[0], r6[2], r6[4]}, d = {r6[1], r6[3], r6[5]};
    const V3 end = o + d;
    const float* A = acts + idx[n] * LUSH_RBK_ACT_STRIDE;
    float* out = new_rays + (long long)n * (M + 1) * 6;
    out[0] = o.x; out[1] = d.x; out[2] = o.y; out[3] = d.y; out[4] = o.z; out[5] = d.z;
    for (int m = 0; m < M; ++m) {   // r.reshape(N,3,M): component c of motion m is column c*M+m (models/lushnerf.py:76)
        const V3 r = {A[RA_R + m], A[RA_R + M + m], A[RA_R + 2 * M + m]};
        const V3 v = {A[RA_V + m], A[RA_V + M + m], A[RA_V + 2 * M + m]};
        const Se3 q = se3_setup(r, v);
        const V3 wo = se3_apply(q, o), we = se3_apply(q, end);
        const V3 wd = we - wo;
        float* w6 = out + (m + 1) * 6;
        w6[0] = wo.x; w6[1] = wd.x; w6[2] = wo.y; w6[3] = wd.y; w6[4] = wo.z; w6[5] = wd.z;
    }
    for (int m = 0; m <= M; ++m) ccw[(long long)n * (M + 1) + m] = A[RA_WN + m];
}

__global__ void rbk_warp_bwd_kernel(const float* __restrict__ rays, const int64_t* __restrict__ idx, int N, int M,
                                    const float* __restrict__ acts, const float* __restrict__ dnew,
                                    const float* __restrict__ dccw, const uint8_t* __restrict__ mask,
                                    float* __restrict__ d_rvw, int rvw_stride, float* __restrict__ drays) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const long long img = idx[n];
    float* G = d_rvw + img * rvw_stride;
    if (dccw)
        for (int m = 0; m <= M; ++m) atomicAdd(G + 24 + m, dccw[(long long)n * (M + 1) + m]);
    const bool live = dnew != nullptr && (mask == nullptr || mask[n] != 0);
    V3 go = {0.f, 0.f, 0.f}, gd = {0.f, 0.f, 0.f};
    if (live) {
        const float* r6 = rays + (long long)n * 6;
        const V3 o = {r6[0], r6[2], r6[4]}, d = {r6[1], r6[3], r6[5]};
        const V3 end = o + d;
        const float* A = acts + img * LUSH_RBK_ACT_STRIDE;
        const float* g6 = dnew + (long long)n * (M + 1) * 6;
        go = {g6[0], g6[2], g6[4]};
        gd = {g6[1], g6[3], g6[5]};
        for (int m = 0; m < M; ++m) {
            const V3 r = {A[RA_R + m], A[RA_R + M + m], A[RA_R + 2 * M + m]};
            const V3 v = {A[RA_V + m], A[RA_V + M + m], A[RA_V + 2 * M + m]};
            const Se3 q = se3_setup(r, v);
            const float* w6 = g6 + (m + 1) * 6;
            const V3 gwo = {w6[0], w6[2], w6[4]}, gwd = {w6[1], w6[3], w6[5]};
            // wd = we - wo
            const V3 gye = gwd, gyo = gwo - gwd;
            V3 gp_o = {0, 0, 0}, gp_e = {0, 0, 0}, gw = {0, 0, 0}, gnu = {0, 0, 0};
            float gth = 0.f, gs = 0.f, gc = 0.f;
            se3_apply_bwd(q, o, gyo, gp_o, gw, gnu, gth, gs, gc);
            se3_apply_bwd(q, end, gye, gp_e, gw, gnu, gth, gs, gc);
            V3 gr, gv;
            se3_finish_bwd(q, r, gw, gnu, gth, gs, gc, gr, gv);
            go = go + gp_o + gp_e;
            gd = gd + gp_e;
            atomicAdd(G + m, gr.x); atomicAdd(G + M + m, gr.y); atomicAdd(G + 2 * M + m, gr.z);
            atomicAdd(G + 12 + m, gv.x); atomicAdd(G + 12 + M + m, gv.y); atomicAdd(G + 12 + 2 * M + m, gv.z);
        }
    }
    if (drays) {
        float* out = drays + (long long)n * 6;
        out[0] = go.x; out[1] = gd.x; out[2] = go.y; out[3] = gd.y; out[4] = go.z; out[5] = gd.z;
    }
}

// ------------------------------------------------- warp + NDC + pack in one (SURVEY 7.2 `rbk_warp_ndc`)
// Rigid_Blurring_Kernel.rbk_warp (models/lushnerf.py:75-98) followed by the head of render_train_scene (:772-795: view
// directions, ndc_rays helpers:542-562, near / far columns) for the M + 1 rays of every input ray, and the same head for the
// input ray alone (render_train_noise, :827-850): rays [N][3][2] -> batch [N*(M+1)][11], ccw [N][M+1], batch0 [N][11].
// One thread per (input ray, motion slot): the warped rays never exist in memory.
__global__ void rbk_warp_ndc_fwd_kernel(const float* __restrict__ rays, const int64_t* __restrict__ idx, int N, int M,
                                        const float* __restrict__ acts, int ndc, float cx, float cy, float near, float far,
                                        float* __restrict__ batch, float* __restrict__ ccw, float* __restrict__ batch0) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int M1 = M + 1;
    if (t >= (long long)N * M1) return;
    const long long n = t / M1;
    const int m = (int)(t % M1);
    const float* r6 = rays + n * 6;
    const V3 o = {r6[0], r6[2], r6[4]}, d = {r6[1], r6[3], r6[5]};
    const float* A = acts + idx[n] * LUSH_RBK_ACT_STRIDE;
    V3 wo = o, wd = d;
    if (m > 0) {    // r.reshape(N,3,M): component c of motion m-1 is column c*M + m-1 (models/lushnerf.py:76)
        const int k = m - 1;
        const V3 r = {A[RA_R + k], A[RA_R + M + k], A[RA_R + 2 * M + k]};
        const V3 v = {A[RA_V + k], A[RA_V + M + k], A[RA_V + 2 * M + k]};
        const Se3 q = se3_setup(r, v);
        wo = se3_apply(q, o);
        wd = se3_apply(q, o + d) - wo;
    }
    const float oo[3] = {wo.x, wo.y, wo.z}, dd[3] = {wd.x, wd.y, wd.z};
    pack_one(oo, dd, ndc, cx, cy, near, far, batch + t * 11);
    ccw[t] = A[RA_WN + m];
    if (m == 0 && batch0 != nullptr) pack_one(oo, dd, ndc, cx, cy, near, far, batch0 + n * 11);
}

// The same for every pixel of ONE training view, rows sub-frame-major (NeRFAll.render_warped_path, models/lushnerf.py:898-947: get_rays
// :917, mlp_rbk :921-925, the head of render_train_scene :929): c2w [3][4], image_idx [1] (read here: no host read-back) ->
// batch [(M+1)*H*W][11] with row m*H*W + n = sub-frame m of pixel n, centre_rays [M+1][3][2] = the un-packed warped rays of pixel
// (H/2, W/2) (:926; may be NULL).  One thread per (sub-frame, pixel), consecutive threads on consecutive pixels of one sub-frame:
// neither the ray table nor the warped rays exist in memory, and the march's outputs are [M+1][H][W] images as they stand.
// The pixel's ray is gen_rays_image_kernel's expression, the warp rbk_warp_ndc_fwd_kernel's: the rows have the same bits.
__global__ __launch_bounds__(256) void warp_image_fwd_kernel(const float* __restrict__ c2w, int H, int W, float fx, float fy, float kx,
                                        float ky, const int64_t* __restrict__ image_idx, int num_img, int M,
                                        const float* __restrict__ acts, int ndc, float cx, float cy, float near, float far,
                                        float* __restrict__ batch, float* __restrict__ centre_rays) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long HW = (long long)H * W;
    if (t >= HW * (M + 1)) return;
    const int m = (int)(t / HW);
    const long long n = t % HW;
    const int px = (int)(n % W), py = (int)(n / W);
    const float d0 = ((float)px + (0.5f - kx)) / fx;
    const float d1 = -((float)py + (0.5f - ky)) / fy;
    const float d2 = -1.f;
    const V3 o = {c2w[3], c2w[7], c2w[11]};
    const V3 d = {(d0 * c2w[0] + d1 * c2w[1]) + d2 * c2w[2], (d0 * c2w[4] + d1 * c2w[5]) + d2 * c2w[6],
                  (d0 * c2w[8] + d1 * c2w[9]) + d2 * c2w[10]};
    long long img = image_idx[0];
    img = img < 0 ? 0 : (img >= num_img ? num_img - 1 : img);     // memory safety only: the reference would raise an IndexError
    const float* A = acts + img * LUSH_RBK_ACT_STRIDE;
    V3 wo = o, wd = d;
    if (m > 0) {    // r.reshape(N,3,M): component c of motion m-1 is column c*M + m-1 (models/lushnerf.py:76)
        const int k = m - 1;
        const V3 r = {A[RA_R + k], A[RA_R + M + k], A[RA_R + 2 * M + k]};
        const V3 v = {A[RA_V + k], A[RA_V + M + k], A[RA_V + 2 * M + k]};
        const Se3 q = se3_setup(r, v);
        wo = se3_apply(q, o);
        wd = se3_apply(q, o + d) - wo;
    }
    const float oo[3] = {wo.x, wo.y, wo.z}, dd[3] = {wd.x, wd.y, wd.z};
    pack_one(oo, dd, ndc, cx, cy, near, far, batch + t * 11);
    if (centre_rays != nullptr && py == H / 2 && px == W / 2) {
        float* c6 = centre_rays + m * 6;
        c6[0] = wo.x; c6[1] = wd.x; c6[2] = wo.y; c6[3] = wd.y; c6[4] = wo.z; c6[5] = wd.z;
    }
}

// Reverse: dbatch [N*(M+1)][11] (may be NULL: only the weights' gradient), dccw [N][M+1] (may be NULL) -> d_rvw [num_img][stride]
// (accumulated; zeroed by lush_rbk_mlp_fwd), drays [N][3][2] (overwritten; may be NULL).  mask as in rbk_warp_bwd_kernel.
// One thread per (input ray, motion slot), RPB rays per workgroup.  The per-image sums are formed in LDS first (up to WN_IMGS
// images) and leave as one global atomic per touched (image, component) and workgroup: with 4096 rays of 26 images the
// first version's 119 k atomics on 754 words took 33 us.
constexpr int WN_IMGS = 64;
__global__ __launch_bounds__(1024) void rbk_warp_ndc_bwd_kernel(const float* __restrict__ rays, const int64_t* __restrict__ idx, int N, int M,
                                        const float* __restrict__ acts, int ndc, float cx, float cy,
                                        const float* __restrict__ dbatch, const float* __restrict__ dccw,
                                        const uint8_t* __restrict__ mask, float* __restrict__ d_rvw, int rvw_stride,
                                        float* __restrict__ drays, int num_img, int RPB) {
    __shared__ float tab[WN_IMGS][LUSH_RBK_RVW_STRIDE];
    __shared__ float racc[1024 / 2][6];           // d(o, d) of the workgroup's rays (RPB <= 512: M >= 1)
    const int M1 = M + 1;
    const bool in_lds = num_img <= WN_IMGS;
    for (int i = threadIdx.x; i < WN_IMGS * LUSH_RBK_RVW_STRIDE; i += blockDim.x) (&tab[0][0])[i] = 0.f;
    for (int i = threadIdx.x; i < RPB * 6; i += blockDim.x) (&racc[0][0])[i] = 0.f;
    __syncthreads();
    const int lr = threadIdx.x / M1, slot = threadIdx.x % M1;
    const long long n = (long long)blockIdx.x * RPB + lr;
    const long long img = (lr < RPB && n < N) ? idx[n] : -1;
    if (img >= 0 && img < num_img) {          // (an index outside the table contributes nothing instead of writing outside it)
        float* G = in_lds ? &tab[img][0] : d_rvw + img * rvw_stride;
        if (dccw) atomicAdd(G + 24 + slot, dccw[n * M1 + slot]);
        const bool live = dbatch != nullptr && (mask == nullptr || mask[n] != 0);
        if (live) {
            const float* r6 = rays + n * 6;
            const V3 o = {r6[0], r6[2], r6[4]}, d = {r6[1], r6[3], r6[5]};
            const float* g11 = dbatch + (n * M1 + slot) * 11;
            V3 go, gd;
            if (slot == 0) {    // the input ray itself
                const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
                float a[3], b[3];
                pack_one_bwd(oo, dd, ndc, cx, cy, g11, a, b);
                go = {a[0], a[1], a[2]};
                gd = {b[0], b[1], b[2]};
            } else {
                const int m = slot - 1;
                const V3 end = o + d;
                const float* A = acts + img * LUSH_RBK_ACT_STRIDE;
                const V3 r = {A[RA_R + m], A[RA_R + M + m], A[RA_R + 2 * M + m]};
                const V3 v = {A[RA_V + m], A[RA_V + M + m], A[RA_V + 2 * M + m]};
                const Se3 q = se3_setup(r, v);
                const V3 wo = se3_apply(q, o), wd = se3_apply(q, end) - wo;     // (recomputed: the warped rays were never stored)
                const float oo[3] = {wo.x, wo.y, wo.z}, dd[3] = {wd.x, wd.y, wd.z};
                float a[3], b[3];
                pack_one_bwd(oo, dd, ndc, cx, cy, g11, a, b);
                const V3 gwo = {a[0], a[1], a[2]}, gwd = {b[0], b[1], b[2]};
                const V3 gye = gwd, gyo = gwo - gwd;       // wd = we - wo
                V3 gp_o = {0, 0, 0}, gp_e = {0, 0, 0}, gw = {0, 0, 0}, gnu = {0, 0, 0};
                float gth = 0.f, gs = 0.f, gc = 0.f;
                se3_apply_bwd(q, o, gyo, gp_o, gw, gnu, gth, gs, gc);
                se3_apply_bwd(q, end, gye, gp_e, gw, gnu, gth, gs, gc);
                V3 gr, gv;
                se3_finish_bwd(q, r, gw, gnu, gth, gs, gc, gr, gv);
                go = gp_o + gp_e;
                gd = gp_e;
                atomicAdd(G + m, gr.x); atomicAdd(G + M + m, gr.y); atomicAdd(G + 2 * M + m, gr.z);
                atomicAdd(G + 12 + m, gv.x); atomicAdd(G + 12 + M + m, gv.y); atomicAdd(G + 12 + 2 * M + m, gv.z);
            }
            if (drays) {
                atomicAdd(&racc[lr][0], go.x); atomicAdd(&racc[lr][1], gd.x); atomicAdd(&racc[lr][2], go.y);
                atomicAdd(&racc[lr][3], gd.y); atomicAdd(&racc[lr][4], go.z); atomicAdd(&racc[lr][5], gd.z);
            }
        }
    }
    __syncthreads();
    if (in_lds)
        for (int i = threadIdx.x; i < num_img * LUSH_RBK_RVW_STRIDE; i += blockDim.x) {
            const float v = (&tab[0][0])[i];
            if (v != 0.f) atomicAdd(d_rvw + (long long)(i / LUSH_RBK_RVW_STRIDE) * rvw_stride + i % LUSH_RBK_RVW_STRIDE, v);
        }
    if (drays)
        for (int i = threadIdx.x; i < RPB * 6; i += blockDim.x) {
            const long long nn = (long long)blockIdx.x * RPB + i / 6;
            if (nn < N) drays[nn * 6 + i % 6] = (&racc[0][0])[i];
        }
}

// ------------------------------------------------------------------- RBK MLP
// y[i][o] = act(b[o] + sum_k W[o][k] x[i][k]) for a few dozen images through ten small dense stages (4 MFLOP in all).
// A workgroup of RBK_NT threads takes RBK_IPB images; their activation rows (512 floats each) live in LDS for the whole
// kernel with an ODD row stride (RBK_LS), and every stage's matrix is copied into LDS once at the head of the kernel.
//
// What these kernels cost was never arithmetic or LDS bandwidth but DEPENDENT LATENCIES IN SERIES, one wave per SIMD with
// nothing to switch to: as `for (t = threadIdx.x; t < count; t += blockDim.x) lds[..] = W[t]` with a run-time trip count the
// compiler emits load, s_waitcnt vmcnt(0), ds_write per iteration, so the 23.8 K weight floats were 93 global-memory round
// trips one after the other (0.3-0.4 us each: the 37 us of the forward, whatever the number of workgroups, staging depth or
// summation batching -- round 4 measured five such variants at 36-39 us before finding this), and the per-image sums of
// the backward's weight gradients were 16 x 4 LDS round trips in series per stage.  Hence the compile-time thread count and
// image count below: every loop has a constant trip count, is fully unrolled with its loads in front of its uses, and rows
// of absent images (n < RBK_IPB) hold zeros instead of shortening a loop.
constexpr int RBK_LS = LUSH_RBK_ACT_STRIDE + 1;
constexpr int RBK_NT = 256;       // threads per workgroup
constexpr int RBK_IPB = 4;        // images per workgroup
constexpr int RBK_WALL = 4 * 64 * 65 + 3 * 32 * 65 + 29 * 33;      // floats of every stage's matrix at row pitch IN + 1 (num_motion <= 4)
constexpr int RBK_FETCH = 16;     // floats per thread of one matrix fetch (64 x 64 / RBK_NT)

// global -> registers (up to RBK_FETCH x RBK_NT floats of W, coalesced), then registers -> LDS at row pitch IN + 1: two calls,
// so that the fetches of SEVERAL matrices are all in flight before the first one is waited for
template <int IN>
__device__ __forceinline__ void rbk_fetch(const float* __restrict__ W, int OUT, float (&v)[RBK_FETCH]) {
#pragma unroll
    for (int j = 0; j < RBK_FETCH; ++j) {
        const int t = j * RBK_NT + threadIdx.x;
        v[j] = t < OUT * IN ? W[t] : 0.f;
    }
}
template <int IN>
__device__ __forceinline__ void rbk_put(float* __restrict__ wb, int OUT, const float (&v)[RBK_FETCH]) {
#pragma unroll
    for (int j = 0; j < RBK_FETCH; ++j) {
        const int t = j * RBK_NT + threadIdx.x;
        if (t < OUT * IN) wb[(t / IN) * (IN + 1) + t % IN] = v[j];
    }
}
struct RbkStages {       // the ten matrices of one pass in the order the pass uses them
    const float* W[10];
    const float* B[10];      // biases (forward only): kept in the pad column of the staged matrix, wb[o * (IN + 1) + IN]
    int OUT[10];
    int WO[10];              // float offset of the staged matrix in the wall
};
// IN of stage st is 64 for st in [first64, first64 + 7), 32 for the other three (forward: 64s first; backward: 32s first)
template <bool BIAS, int FIRST64>
__device__ __forceinline__ void rbk_stage_all(RbkStages& S, float* __restrict__ wall) {
    int off = 0;
#pragma unroll
    for (int st = 0; st < 10; ++st) {
        S.WO[st] = off;
        off += S.OUT[st] * ((st >= FIRST64 && st < FIRST64 + 7 ? 64 : 32) + 1);
    }
    float bias[10];
    if (BIAS) {
#pragma unroll
        for (int st = 0; st < 10; ++st) bias[st] = (int)threadIdx.x < S.OUT[st] ? S.B[st][threadIdx.x] : 0.f;
    }
    // every matrix's fetch in flight before the first is waited for (160 registers of fetched weights; one wave per SIMD has 512)
    {
        float v[10][RBK_FETCH];
#pragma unroll
        for (int st = 0; st < 10; ++st) {
            if (st >= FIRST64 && st < FIRST64 + 7) rbk_fetch<64>(S.W[st], S.OUT[st], v[st]);
            else rbk_fetch<32>(S.W[st], S.OUT[st], v[st]);
        }
#pragma unroll
        for (int st = 0; st < 10; ++st) {
            if (st >= FIRST64 && st < FIRST64 + 7) rbk_put<64>(wall + S.WO[st], S.OUT[st], v[st]);
            else rbk_put<32>(wall + S.WO[st], S.OUT[st], v[st]);
        }
    }
    if (BIAS) {
#pragma unroll
        for (int st = 0; st < 10; ++st) {
            const int in = st >= FIRST64 && st < FIRST64 + 7 ? 64 : 32;
            if ((int)threadIdx.x < S.OUT[st]) wall[S.WO[st] + threadIdx.x * (in + 1) + in] = bias[st];
        }
    }
}

// y[i][o] = act(b[o] + sum_k W[o][k] x[i][k]) from the staged W: bias first, k ascending (the order of every earlier version);
// RBK_IPB x OUT <= RBK_NT outputs, one per thread, image index fastest across lanes
template <int IN>
__device__ __forceinline__ void rbk_dense_lds(const float* __restrict__ wb, const float* x, float* y, int OUT, int relu) {
    const int i = threadIdx.x % RBK_IPB, o = threadIdx.x / RBK_IPB;
    if (o >= OUT) return;
    const float* w = wb + o * (IN + 1);
    const float* xi = x + i * RBK_LS;
    float s = w[IN];
#pragma unroll
    for (int k0 = 0; k0 < IN; k0 += 16) {       // (operands of 16 terms fetched before they are summed)
        float wv[16], xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) { wv[j] = w[k0 + j]; xv[j] = xi[k0 + j]; }
#pragma unroll
        for (int j = 0; j < 16; ++j) s += wv[j] * xv[j];
    }
    y[i * RBK_LS + o] = relu ? fmaxf(s, 0.f) : s;
}

__global__ __launch_bounds__(RBK_NT) void rbk_mlp_fwd_kernel(lush_rbk_params p, int n_all, int M, float window,
                                                            float* __restrict__ acts) {
    const int img0 = blockIdx.x * RBK_IPB;
    const int n = n_all - img0 < RBK_IPB ? n_all - img0 : RBK_IPB;
    p.embed += (long long)img0 * 64;
    acts += (long long)img0 * LUSH_RBK_ACT_STRIDE;
    extern __shared__ float rbk_lds[];
    float* A = rbk_lds;                             // [RBK_IPB][RBK_LS] activations
    float* wall = rbk_lds + RBK_IPB * RBK_LS;       // every stage's matrix
    constexpr int ST = LUSH_RBK_ACT_STRIDE;
    RbkStages S = {{p.w_trunk[0], p.w_trunk[1], p.w_trunk[2], p.w_trunk[3], p.w_rb, p.w_vb, p.w_wb, p.w_r, p.w_v, p.w_w},
                   {p.b_trunk[0], p.b_trunk[1], p.b_trunk[2], p.b_trunk[3], p.b_rb, p.b_vb, p.b_wb, p.b_r, p.b_v, p.b_w},
                   {64, 64, 64, 64, 32, 32, 32, 3 * M, 3 * M, M + 1}, {}};
    const int XO[10] = {RA_E, RA_H0, RA_H0 + 64, RA_H0 + 128, RA_H0 + 192, RA_H0 + 192, RA_H0 + 192, RA_HR, RA_HV, RA_HW};
    const int YO[10] = {RA_H0, RA_H0 + 64, RA_H0 + 128, RA_H0 + 192, RA_HR, RA_HV, RA_HW, RA_R, RA_V, RA_WS};
    {   // (RBK_IPB x 64 = RBK_NT: one embedding float per thread; an absent image's row is zeros and is never written out)
        const int i = threadIdx.x / 64;
        A[i * RBK_LS + RA_E + threadIdx.x % 64] = i < n ? p.embed[threadIdx.x] : 0.f;
    }
    rbk_stage_all<true, 0>(S, wall);
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 10; ++st) {
        if (st < 7) rbk_dense_lds<64>(wall + S.WO[st], A + XO[st], A + YO[st], S.OUT[st], 1);
        else rbk_dense_lds<32>(wall + S.WO[st], A + XO[st], A + YO[st], S.OUT[st], 0);
        // (the three branches and the three heads read one input and write disjoint outputs: one barrier per group)
        if (st != 4 && st != 5 && st != 7 && st != 8) __syncthreads();
    }
    if ((int)threadIdx.x < RBK_IPB * 3 * M) {
        const int i = threadIdx.x / (3 * M), o = threadIdx.x % (3 * M);
        A[i * RBK_LS + RA_R + o] *= window;
        A[i * RBK_LS + RA_V + o] *= window;
    }
    if ((int)threadIdx.x < RBK_IPB) {
        const int i = threadIdx.x;
        float sum = 0.f;
        for (int m = 0; m <= M; ++m) {
            const float s = 1.f / (1.f + expf(-A[i * RBK_LS + RA_WS + m]));
            A[i * RBK_LS + RA_WS + m] = s;
            sum += s;
        }
        for (int m = 0; m <= M; ++m) A[i * RBK_LS + RA_WN + m] = A[i * RBK_LS + RA_WS + m] / (sum + 1e-10f);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RBK_IPB * ST / RBK_NT; ++j) {
        const int t = j * RBK_NT + threadIdx.x;
        if (t < n * ST) acts[t] = (t % ST) < RA_WN + 8 ? A[(t / ST) * RBK_LS + (t % ST)] : 0.f;
    }
}

// dx[i][k] = [gate[i][k] > 0] * (sum_o W[o][k] dz[i][o] (+ dx[i][k])) from the staged W (row pitch IN + 1); o ascending, the
// previous value added last, the gate applied to the total -- the arithmetic of round 3's separate passes.
// RBK_IPB x IN <= RBK_NT outputs, one per thread.
template <int IN>
__device__ __forceinline__ void rbk_dense_bwd_x_lds(const float* __restrict__ wb, const float* dz, float* dx, const float* gate,
                                                    int OUT, int accumulate) {
    const int i = threadIdx.x % RBK_IPB, k = threadIdx.x / RBK_IPB;
    if (k >= IN) return;
    float s = 0.f;
    const float* zi = dz + i * RBK_LS;
    int o0 = 0;
    for (; o0 + 8 <= OUT; o0 += 8) {          // (operands of 8 terms fetched before they are summed; same order of the sum)
        float wv[8], zv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { wv[j] = wb[(o0 + j) * (IN + 1) + k]; zv[j] = zi[o0 + j]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) s += wv[j] * zv[j];
    }
    if (o0 < OUT) {                            // the heads' 3 M or M + 1 outputs: up to 7 more, fetched together as well
        float wv[8], zv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = o0 + j < OUT;
            wv[j] = in ? wb[(o0 + j) * (IN + 1) + k] : 0.f;
            zv[j] = in ? zi[o0 + j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (o0 + j < OUT) s += wv[j] * zv[j];
    }
    if (accumulate) s += dx[i * RBK_LS + k];
    if (gate && !(gate[i * RBK_LS + k] > 0.f)) s = 0.f;
    dx[i * RBK_LS + k] = s;
}
// dW[o][k] += sum_i dz[i][o] x[i][k], db[o] += sum_i dz[i][o]: added into buffers that hold values (the trainer's flat gradient,
// or zeros the launcher wrote), by atomics because several workgroups -- each with its own images -- add into the same matrix.
// Thread t takes outputs t, t + RBK_NT, ...: k = t % IN is the same for all of them (RBK_NT is a multiple of IN), so a thread
// reads its RBK_IPB activations once; rows of absent images hold zeros.
template <int IN>
__device__ __forceinline__ void rbk_dense_bwd_w(const float* dz, const float* x, float* __restrict__ dW, float* __restrict__ db, int OUT) {
    const int k = threadIdx.x % IN, o_first = threadIdx.x / IN;
    constexpr int OSTEP = RBK_NT / IN;
    float xv[RBK_IPB];
#pragma unroll
    for (int i = 0; i < RBK_IPB; ++i) xv[i] = x[i * RBK_LS + k];
#pragma unroll
    for (int r = 0; r < 64 / OSTEP; ++r) {
        const int o = o_first + r * OSTEP;
        if (o < OUT) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < RBK_IPB; ++i) s += dz[i * RBK_LS + o] * xv[i];
            atomicAdd(dW + o * IN + k, s);
        }
    }
    if ((int)threadIdx.x < OUT) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < RBK_IPB; ++i) s += dz[i * RBK_LS + threadIdx.x];
        atomicAdd(db + threadIdx.x, s);
    }
    // (no barrier: dW / db are outputs only; the adjoints a later stage overwrites are guarded by that stage's barrier)
}

// Workgroup b takes images [b RBK_IPB, (b + 1) RBK_IPB): d(activation) is per image, the weight gradients are sums over images.
__global__ __launch_bounds__(RBK_NT) void rbk_mlp_bwd_kernel(lush_rbk_params p, int n_all, int M, float window,
                                                            const float* __restrict__ acts,
                                                            float* __restrict__ d_rvw, lush_rbk_grads g,
                                                            int RS /* floats between two images' rows of d_rvw */) {
    const int img0 = blockIdx.x * RBK_IPB;
    const int n = n_all - img0 < RBK_IPB ? n_all - img0 : RBK_IPB;
    acts += (long long)img0 * LUSH_RBK_ACT_STRIDE;
    d_rvw += (long long)img0 * RS;
    g.embed += (long long)img0 * 64;
    // LDS: activations [RBK_IPB][RBK_LS], then the adjoints of the pre-activations in the same per-image layout, then the matrices
    extern __shared__ float rbk_lds[];
    float* A = rbk_lds;
    float* sc = rbk_lds + RBK_IPB * RBK_LS;
    float* wall = rbk_lds + 2 * RBK_IPB * RBK_LS;
    constexpr int ST = LUSH_RBK_ACT_STRIDE;
    {
        float v[RBK_IPB * ST / RBK_NT];
#pragma unroll
        for (int j = 0; j < RBK_IPB * ST / RBK_NT; ++j) {
            const int t = j * RBK_NT + threadIdx.x;
            v[j] = t < n * ST ? acts[t] : 0.f;            // (an absent image: zero activations, zero adjoints)
        }
#pragma unroll
        for (int j = 0; j < RBK_IPB * ST / RBK_NT; ++j) {
            const int t = j * RBK_NT + threadIdx.x;
            A[(t / ST) * RBK_LS + (t % ST)] = v[j];
            sc[(t / ST) * RBK_LS + (t % ST)] = 0.f;
        }
    }
    // ten dx stages: heads r, v, w; branches rb, vb, wb into one d h3; trunk 3..0
    RbkStages S = {{p.w_r, p.w_v, p.w_w, p.w_rb, p.w_vb, p.w_wb, p.w_trunk[3], p.w_trunk[2], p.w_trunk[1], p.w_trunk[0]}, {},
                   {3 * M, 3 * M, M + 1, 32, 32, 32, 64, 64, 64, 64}, {}};
    rbk_stage_all<false, 3>(S, wall);
    __syncthreads();
    if ((int)threadIdx.x < RBK_IPB * 3 * M) {
        const int i = threadIdx.x / (3 * M), o = threadIdx.x % (3 * M);
        if (i < n) {
            sc[i * RBK_LS + RA_R + o] = d_rvw[i * RS + o] * window;
            sc[i * RBK_LS + RA_V + o] = d_rvw[i * RS + 12 + o] * window;
            // consumed: every element of d_rvw is read by exactly one thread, which leaves it ZERO -- the rows live in the zero
            // tail of `acts` (LUSH_RBK_RVW_OFFSET), so a second backward over the same saved activations starts from zero again
            d_rvw[i * RS + o] = 0.f;
            d_rvw[i * RS + 12 + o] = 0.f;
        }
    }
    if ((int)threadIdx.x < n) {
        const int i = threadIdx.x;
        float sum = 1e-10f, dotp = 0.f;
        for (int m = 0; m <= M; ++m) { sum += A[i * RBK_LS + RA_WS + m]; dotp += d_rvw[i * RS + 24 + m] * A[i * RBK_LS + RA_WS + m]; }
        for (int m = 0; m <= M; ++m) {
            const float ws = A[i * RBK_LS + RA_WS + m];
            const float dws = d_rvw[i * RS + 24 + m] / sum - dotp / (sum * sum);
            sc[i * RBK_LS + RA_WS + m] = dws * ws * (1.f - ws);
            d_rvw[i * RS + 24 + m] = 0.f;
        }
    }
    __syncthreads();
    const int ZO[10] = {RA_R, RA_V, RA_WS, RA_HR, RA_HV, RA_HW, RA_H0 + 192, RA_H0 + 128, RA_H0 + 64, RA_H0};
    const int XO[10] = {RA_HR, RA_HV, RA_HW, RA_H0 + 192, RA_H0 + 192, RA_H0 + 192, RA_H0 + 128, RA_H0 + 64, RA_H0, RA_E};
    const int GATE[10] = {1, 1, 1, 0, 0, 1, 1, 1, 1, 0};       // ReLU gate of the stage's input activations (d h3: after the third addend)
    const int ACC[10] = {0, 0, 0, 0, 1, 1, 0, 0, 0, 0};
    float* gw[10] = {g.w_r, g.w_v, g.w_w, g.w_rb, g.w_vb, g.w_wb, g.w_trunk[3], g.w_trunk[2], g.w_trunk[1], g.w_trunk[0]};
    float* gb[10] = {g.b_r, g.b_v, g.b_w, g.b_rb, g.b_vb, g.b_wb, g.b_trunk[3], g.b_trunk[2], g.b_trunk[1], g.b_trunk[0]};
#pragma unroll
    for (int st = 0; st < 10; ++st) {
        // dW / db of this stage: dz (complete since the previous barrier) x the stage's input activations
        if (st < 3) {
            rbk_dense_bwd_w<32>(sc + ZO[st], A + XO[st], gw[st], gb[st], S.OUT[st]);
            rbk_dense_bwd_x_lds<32>(wall + S.WO[st], sc + ZO[st], sc + XO[st], GATE[st] ? A + XO[st] : nullptr, S.OUT[st], ACC[st]);
        } else {
            rbk_dense_bwd_w<64>(sc + ZO[st], A + XO[st], gw[st], gb[st], S.OUT[st]);
            rbk_dense_bwd_x_lds<64>(wall + S.WO[st], sc + ZO[st], sc + XO[st], GATE[st] ? A + XO[st] : nullptr, S.OUT[st], ACC[st]);
        }
        // (the three heads write three different adjoints: one barrier behind them; the three branches accumulate into ONE d h3
        // in order, a barrier each)
        if (st != 0 && st != 1) __syncthreads();
    }
    {   // (an image's embedding row belongs to one workgroup; RBK_IPB x 64 = RBK_NT)
        const int i = threadIdx.x / 64;
        if (i < n) g.embed[threadIdx.x] += sc[i * RBK_LS + RA_E + (threadIdx.x % 64)];
    }
}

}  // namespace lush

using namespace lush;

extern "C" {

int lush_rbk_mlp_fwd(const lush_rbk_params* p, int num_img, int M, float window, float* acts, lush_stream_t st) {
    if (M < 1 || M > 4) return set_error("lush_rbk_mlp_fwd: 1 <= num_motion <= 4");
    if (num_img < 1) return set_error("lush_rbk_mlp_fwd: no images");
    const size_t lds = ((size_t)RBK_IPB * RBK_LS + RBK_WALL) * sizeof(float);
    LUSH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rbk_mlp_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return launch(rbk_mlp_fwd_kernel, dim3(cdiv(num_img, RBK_IPB)), dim3(RBK_NT), lds, st, *p, num_img, M, window, acts);
}
int lush_rbk_mlp_bwd(const lush_rbk_params* p, int num_img, int M, float window, const float* acts,
                     float* d_rvw, int rvw_stride, const lush_rbk_grads* g, float* scratch, int accumulate, lush_stream_t st) {
    if (M < 1 || M > 4) return set_error("lush_rbk_mlp_bwd: 1 <= num_motion <= 4");
    if (num_img < 1) return set_error("lush_rbk_mlp_bwd: no images");
    if (rvw_stride < LUSH_RBK_RVW_STRIDE) return set_error("lush_rbk_mlp_bwd: rvw_stride must be at least LUSH_RBK_RVW_STRIDE");
    // the weight gradients are summed by atomics into buffers that hold values -- the trainer's flat gradient (accumulate != 0),
    // or zeros written here first (accumulate == 0: 19 small memsets, not a path a training step takes)
    if (!accumulate) {
        const size_t f = sizeof(float);
        const hipStream_t s = (hipStream_t)st;
        LUSH_HIP(hipMemsetAsync(g->embed, 0, (size_t)num_img * 64 * f, s));
        for (int l = 0; l < 4; ++l) {
            LUSH_HIP(hipMemsetAsync(g->w_trunk[l], 0, 64 * 64 * f, s));
            LUSH_HIP(hipMemsetAsync(g->b_trunk[l], 0, 64 * f, s));
        }
        float* w32[3] = {g->w_rb, g->w_vb, g->w_wb};
        float* b32[3] = {g->b_rb, g->b_vb, g->b_wb};
        for (int i = 0; i < 3; ++i) {
            LUSH_HIP(hipMemsetAsync(w32[i], 0, 32 * 64 * f, s));
            LUSH_HIP(hipMemsetAsync(b32[i], 0, 32 * f, s));
        }
        LUSH_HIP(hipMemsetAsync(g->w_r, 0, (size_t)3 * M * 32 * f, s)); LUSH_HIP(hipMemsetAsync(g->b_r, 0, (size_t)3 * M * f, s));
        LUSH_HIP(hipMemsetAsync(g->w_v, 0, (size_t)3 * M * 32 * f, s)); LUSH_HIP(hipMemsetAsync(g->b_v, 0, (size_t)3 * M * f, s));
        LUSH_HIP(hipMemsetAsync(g->w_w, 0, (size_t)(M + 1) * 32 * f, s)); LUSH_HIP(hipMemsetAsync(g->b_w, 0, (size_t)(M + 1) * f, s));
    }
    (void)scratch;      // (unused since the LDS version; kept in the signature)
    const size_t lds = ((size_t)2 * RBK_IPB * RBK_LS + RBK_WALL) * sizeof(float);
    LUSH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rbk_mlp_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return launch(rbk_mlp_bwd_kernel, dim3(cdiv(num_img, RBK_IPB)), dim3(RBK_NT), lds, st, *p, num_img, M, window, acts, d_rvw, *g,
                  rvw_stride);
}
int lush_rbk_warp_fwd(const float* rays, const int64_t* idx, int N, int M, const float* acts, float* new_rays,
                      float* ccw, lush_stream_t st) {
    return launch(rbk_warp_fwd_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, rays, idx, N, M, acts, new_rays, ccw);
}
int lush_rbk_warp_bwd(const float* rays, const int64_t* idx, int N, int M, const float* acts, const float* dnew_rays,
                      const float* dccw, const uint8_t* mask, float* d_rvw, int rvw_stride, float* drays, lush_stream_t st) {
    if (rvw_stride < LUSH_RBK_RVW_STRIDE) return set_error("lush_rbk_warp_bwd: rvw_stride must be at least LUSH_RBK_RVW_STRIDE");
    return launch(rbk_warp_bwd_kernel, dim3(cdiv(N, 128)), dim3(128), 0, st, rays, idx, N, M, acts, dnew_rays, dccw, mask, d_rvw, rvw_stride, drays);
}

int lush_rbk_warp_ndc_fwd(const float* rays, const int64_t* idx, int N, int M, const float* acts, int ndc, float cx, float cy,
                          float near, float far, float* batch, float* ccw, float* batch0, lush_stream_t st) {
    if (N < 1 || M < 1 || M > 4) return set_error("lush_rbk_warp_ndc_fwd: need N >= 1 and 1 <= num_motion <= 4");
    if (!rays || !idx || !acts || !batch || !ccw) return set_error("lush_rbk_warp_ndc_fwd: rays, idx, acts, batch and ccw are required");
    return launch(rbk_warp_ndc_fwd_kernel, dim3(cdiv((long long)N * (M + 1), 256)), dim3(256), 0, st, rays, idx, N, M, acts, ndc,
                  cx, cy, near, far, batch, ccw, batch0);
}
int lush_warp_image_fwd(const float* c2w, int H, int W, float fx, float fy, float kx, float ky, const int64_t* image_idx, int num_img,
                        int M, const float* acts, int ndc, float cx, float cy, float near, float far, float* batch, float* centre_rays,
                        lush_stream_t st) {
    if (H <= 0 || W <= 0) return set_error("lush_warp_image_fwd: empty image");
    if (M < 1 || M > 4) return set_error("lush_warp_image_fwd: 1 <= num_motion <= 4");
    if (num_img < 1) return set_error("lush_warp_image_fwd: no images");
    const long long rows = (long long)H * W * (M + 1);
    if (rows > 0x7fffffffLL) return set_error("lush_warp_image_fwd: H*W*(num_motion+1) must stay below 2^31 (the march counts its rays in an int)");
    if (!c2w || !image_idx || !acts || !batch) return set_error("lush_warp_image_fwd: c2w, image_idx, acts and batch are required");
    return launch(warp_image_fwd_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, st, c2w, H, W, fx, fy, kx, ky, image_idx, num_img, M,
                  acts, ndc, cx, cy, near, far, batch, centre_rays);
}
int lush_rbk_warp_ndc_bwd(const float* rays, const int64_t* idx, int N, int M, const float* acts, int ndc, float cx, float cy,
                          const float* dbatch, const float* dccw, const uint8_t* mask, float* d_rvw, int rvw_stride, float* drays,
                          int num_img, lush_stream_t st) {
    if (N < 1 || M < 1 || M > 4) return set_error("lush_rbk_warp_ndc_bwd: need N >= 1 and 1 <= num_motion <= 4");
    if (!rays || !idx || !acts || !d_rvw) return set_error("lush_rbk_warp_ndc_bwd: rays, idx, acts and d_rvw are required");
    if (rvw_stride < LUSH_RBK_RVW_STRIDE) return set_error("lush_rbk_warp_ndc_bwd: rvw_stride must be at least LUSH_RBK_RVW_STRIDE");
    if (num_img < 1) return set_error("lush_rbk_warp_ndc_bwd: num_img (the number of rows of acts / d_rvw) must be given");
    const int M1 = M + 1;
    int rpb = 256 / M1;                        // ~256 threads per workgroup: enough workgroups to spread over the chip
    if (rpb > N) rpb = N;
    return launch(rbk_warp_ndc_bwd_kernel, dim3(cdiv(N, rpb)), dim3(rpb * M1), 0, st, rays, idx, N, M, acts, ndc, cx, cy, dbatch,
                  dccw, mask, d_rvw, rvw_stride, drays, num_img, rpb);
}

}  // extern "C"
