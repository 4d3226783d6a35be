// lush-march: the field as a function of points the caller chose, and compositing on the caller's own z
// (NeRFAll.mlpforward / mlpforward_noise / raw2outputs, models/lushnerf.py:234-352) + their C ABI.
//   points_pack_kernel         free points -> the pseudo-rays [pt, 0, 0,1, dir] and z = 0 an MLP launch of (P,1) takes
//   points_grad_kernel         the chain's d(point) rows -> d(points), d(directions) (the sum over a ray's samples)
//   composite_bwd_full_kernel  the complete backward of raw2outputs: all five results, d_raw, d_z, d_rays_d
#include "lush_common.h"
#include "lush_host.h"
#include "lush_composite.h"
#include "../../include/lush_march.h"

namespace lush {

// ---------------------------------------------------------------- free points
// The MLP kernels form a point as o + d*z with a separate multiply and add (-ffp-contract=off): pt + 0*0 reaches the
// encoder with the caller's bits.  near = 0, far = 1 are never read by an MLP launch.
__global__ __launch_bounds__(256) void points_pack_kernel(const float* __restrict__ pts, const float* __restrict__ dirs,
        int R, int S, float* __restrict__ rays, float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)R * S) return;
    const long long ray = i / S;
    float* o = rays + i * 11;
    o[0] = pts[i * 3]; o[1] = pts[i * 3 + 1]; o[2] = pts[i * 3 + 2];
    o[3] = 0.f; o[4] = 0.f; o[5] = 0.f;
    o[6] = 0.f; o[7] = 1.f;
    o[8] = dirs[ray * 3]; o[9] = dirs[ray * 3 + 1]; o[10] = dirs[ray * 3 + 2];
    z[i] = 0.f;
}

// One wavefront per ray, 64 samples per step: a lane adds its samples in the order of the steps, then one wave sum.
// No atomics: two runs give the same bits.
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void points_grad_kernel(const float* __restrict__ dpts, int R, int S,
        float* __restrict__ d_pts, float* __restrict__ d_dirs) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= R) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int s = lane; s < S; s += 64) {
        const long long p = (long long)ray * S + s;
        const float4 gx = *reinterpret_cast<const float4*>(dpts + p * 8);
        const float4 gv = *reinterpret_cast<const float4*>(dpts + p * 8 + 4);
        d_pts[p * 3] = gx.x; d_pts[p * 3 + 1] = gx.y; d_pts[p * 3 + 2] = gx.z;
        a0 += gv.x; a1 += gv.y; a2 += gv.z;
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if (lane < 3) d_dirs[(long long)ray * 3 + lane] = lane == 0 ? a0 : (lane == 1 ? a1 : a2);
}

// ------------------------------------------------- raw2outputs, whole backward
// Upstream gradients of the five results (any may be NULL = 0): rgb_map [R][3], density [R][S-1], acc_map [R],
// weights [R][S], depth_map [R].
struct CompGrads { const float *rgb, *density, *acc, *weights, *depth; };

// With G_j = dL/dw_j = g_rgb.rgb_j + g_depth z_j + g_acc + g_weights_j (g_acc less sum(g_rgb) under white_bkgd) and
// S_j = sum_{k>j} G_k alpha_k prod_{j<m<k} (1 - alpha_m) from composite_bwd_kernel's reverse affine scan (no division by 1 - alpha:
// on a sharp field fp32 rounds many alpha to exactly 1):
//   dL/dalpha_j = T_j (G_j - S_j),  x = sigma dists:  dL/dx_j = dL/dalpha_j (1 - alpha_j)
//   dL/dsigma_raw_j = gate_j (dL/dx_j dists_j + g_density_j)     gate = near mask x 1[raw_sigma + noise > 0]
//   dL/ddists_j = dL/dx_j sigma_j
//   d_z_j = |d| (dL/ddists_{j-1} - dL/ddists_j) + g_depth w_j      (the near mask is a step in z: no gradient)
//   d_rays_d = (sum_j dL/ddists_j (z_{j+1} - z_j)) d / |d|
// The last sample has alpha = 1 whatever its raw sigma: d_raw[.., 3] = 0 there.  Lane l owns samples l*SPL .. l*SPL+SPL-1.
template <int SPL>
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void composite_bwd_full_kernel(CompIn c, CompGrads g, float* __restrict__ d_raw,
        float* __restrict__ d_z, float* __restrict__ d_rays_d) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= c.R) return;      // (wave-uniform: the shuffles below run with all 64 lanes)
    float alpha[SPL], dist[SPL], dens[SPL], gate[SPL], zz[SPL], col[SPL][3], T[SPL], norm;
    comp_load<SPL>(c, ray, lane, alpha, dist, dens, gate, zz, col, norm);
    comp_trans<SPL>(alpha, lane, T);
    float gr[3] = {0.f, 0.f, 0.f};
    if (g.rgb) { gr[0] = g.rgb[ray * 3]; gr[1] = g.rgb[ray * 3 + 1]; gr[2] = g.rgb[ray * 3 + 2]; }
    const float gd = g.depth ? g.depth[ray] : 0.f;
    float ga = g.acc ? g.acc[ray] : 0.f;
    if (c.white_bkgd) ga -= gr[0] + gr[1] + gr[2];
    float G[SPL];
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const int j = lane * SPL + e;
        const float gw = (g.weights && j < c.S) ? g.weights[(long long)ray * c.S + j] : 0.f;
        G[e] = gr[0] * col[e][0] + gr[1] * col[e][1] + gr[2] * col[e][2] + gd * zz[e] + ga + gw;
    }
    // reverse scan of the affine maps f_k(s) = G_k alpha_k + (1 - alpha_k) s: lane aggregate, then the suffix over lanes
    float Fa = 1.f, Fb = 0.f;
#pragma unroll
    for (int e = SPL - 1; e >= 0; --e) {
        Fb = G[e] * alpha[e] + (1.f - alpha[e]) * Fb;
        Fa = (1.f - alpha[e]) * Fa;
    }
    float Sa = Fa, Sb = Fb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ta = __shfl_down(Sa, o, 64), tb = __shfl_down(Sb, o, 64);
        if (lane + o < 64) { Sb = Sa * tb + Sb; Sa = Sa * ta; }
    }
    float sfx = __shfl_down(Sb, 1, 64);      // S_j of the lane's last sample
    if (lane == 63) sfx = 0.f;
    float znext[SPL], ddist[SPL], dnorm = 0.f;
#pragma unroll
    for (int e = 0; e + 1 < SPL; ++e) znext[e] = zz[e + 1];
    znext[SPL - 1] = __shfl_down(zz[0], 1, 64);      // z of the next lane's first sample
#pragma unroll
    for (int e = SPL - 1; e >= 0; --e) {
        const int j = lane * SPL + e;
        const float wgt = alpha[e] * T[e];
        ddist[e] = 0.f;
        if (j < c.S) {
            float4 o;
            o.x = wgt * gr[0] * col[e][0] * (1.f - col[e][0]);
            o.y = wgt * gr[1] * col[e][1] * (1.f - col[e][1]);
            o.z = wgt * gr[2] * col[e][2] * (1.f - col[e][2]);
            o.w = 0.f;
            if (j < c.S - 1) {
                const float dalpha = T[e] * (G[e] - sfx);
                const float om = 1.f - alpha[e];            // = exp(-dens*dist)
                const float gdens = g.density ? g.density[(long long)ray * (c.S - 1) + j] : 0.f;
                o.w = gate[e] * (dalpha * om * dist[e] + gdens);
                ddist[e] = dalpha * om * dens[e];
                dnorm += ddist[e] * (znext[e] - zz[e]);
            }
            *reinterpret_cast<float4*>(d_raw + ((long long)ray * c.S + j) * 4) = o;
        }
        sfx = G[e] * alpha[e] + (1.f - alpha[e]) * sfx;     // becomes S_{j-1}
    }
    float ddist_before = __shfl_up(ddist[SPL - 1], 1, 64);      // dL/ddists of the sample before this lane's first
    if (lane == 0) ddist_before = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const int j = lane * SPL + e;
        if (j < c.S) d_z[(long long)ray * c.S + j] = norm * (ddist_before - ddist[e]) + gd * (alpha[e] * T[e]);
        ddist_before = ddist[e];
    }
    dnorm = wave_sum(dnorm);
    if (lane < 3) d_rays_d[(long long)ray * 3 + lane] = norm > 0.f ? dnorm * c.rays[(long long)ray * 11 + 3 + lane] / norm : 0.f;
}

}  // namespace lush

using namespace lush;

extern "C" {

int lush_points_pack(const float* pts, const float* dirs, int R, int S, float* rays, float* z, lush_stream_t st) {
    if (R <= 0 || S <= 0) return set_error("lush_points_pack: empty");
    if (!pts || !dirs || !rays || !z) return set_error("lush_points_pack: points, directions and both outputs are required");
    if ((long long)R * S >= (1LL << 27)) return set_error("lush_points_pack: R * S must be below 2^27 points (what one MLP launch takes)");
    return launch(points_pack_kernel, dim3(cdiv((long long)R * S, 256)), dim3(256), 0, st, pts, dirs, R, S, rays, z);
}

int lush_points_grad(const float* dpts, int R, int S, float* d_pts, float* d_dirs, lush_stream_t st) {
    if (R <= 0 || S <= 0) return set_error("lush_points_grad: empty");
    if (!dpts || !d_pts || !d_dirs) return set_error("lush_points_grad: the d(point) rows and both outputs are required");
    if ((long long)R * S >= (1LL << 27)) return set_error("lush_points_grad: R * S must be below 2^27 points (what one MLP launch takes)");
    return launch(points_grad_kernel, dim3(cdiv(R, RAYS_PER_BLOCK)), dim3(RAYS_PER_BLOCK * 64), 0, st, dpts, R, S, d_pts, d_dirs);
}

int lush_composite_bwd_full(const float* raw, const float* z, const float* rays, int R, int S, const float* noise,
                            float noise_std, float near_mask, int white_bkgd, const float* g_rgb, const float* g_density,
                            const float* g_acc, const float* g_weights, const float* g_depth, float* d_raw, float* d_z,
                            float* d_rays_d, lush_stream_t st) {
    if (S < 2 || S > 256) return set_error("lush_composite_bwd_full: S must be in [2,256]");
    if (R <= 0) return set_error("lush_composite_bwd_full: empty");
    if (!raw || !z || !rays || !d_raw || !d_z || !d_rays_d) return set_error("lush_composite_bwd_full: raw, z, rays and the three outputs are required");
    const CompIn c{raw, z, rays, noise, R, S, noise_std, near_mask, white_bkgd};
    const CompGrads g{g_rgb, g_density, g_acc, g_weights, g_depth};
    const dim3 grid(cdiv(R, RAYS_PER_BLOCK)), block(RAYS_PER_BLOCK * 64);
    return comp_for_spl(S, [&](auto spl) {
        return launch(composite_bwd_full_kernel<decltype(spl)::value>, grid, block, 0, st, c, g, d_raw, d_z, d_rays_d); });
}

}  // extern "C"
