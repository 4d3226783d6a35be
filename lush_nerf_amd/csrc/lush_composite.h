// lush-march: what the compositing kernels share (lush_march.hip: forward and the march's backward; lush_field.hip: the
// complete backward of raw2outputs) -- the per-lane loads of a ray and its transmittance, so that every one of them sees the
// alpha, T and weights the forward computed, bit for bit.
#pragma once
#include "lush_common.h"
#include <type_traits>

namespace lush {

constexpr int RAYS_PER_BLOCK = 4;   // 4 waves per workgroup, one ray each

// ---------------------------------------------------------------- compositing
// Lane l owns samples l*SPL .. l*SPL+SPL-1.
struct CompIn {
    const float *raw, *z, *rays, *noise;
    int R, S;
    float noise_std, near_mask;
    int white_bkgd;
};
// host: f(std::integral_constant<int, SPL>) for the SPL of a ray of S <= 256 samples
template <class F>
int comp_for_spl(int S, F&& f) {
    if (S <= 64) return f(std::integral_constant<int, 1>{});
    if (S <= 128) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}

// The one statement of which samples before the last pass density on: the clamp of raw2outputs (pre = raw sigma + noise) and
// near_mask.  A sample that fails it has density 0, alpha 0, weight 0 and an exactly zero d_raw row.  comp_load and the forward's
// live list (live_fwd_pred, lush_march.hip) both ask here: a point the list missed would keep colour 0 at a non-zero weight.
__device__ __forceinline__ bool comp_gate(float pre, float znext, float near_mask) {
    return pre > 0.f && !(near_mask >= 0.f && !(znext > near_mask));
}
// pre-activation of sample j < S-1 of a ray as the compositing sees it
__device__ __forceinline__ float comp_pre(float sigma, const float* noise, float noise_std, long long ray, int S, int j) {
    float pre = sigma;
    if (noise != nullptr && noise_std > 0.f) pre += noise[ray * (S - 1) + j] * noise_std;
    return pre;
}

template <int SPL>
__device__ __forceinline__ void comp_load(const CompIn& c, int ray, int lane, float (&alpha)[SPL], float (&dist)[SPL],
                                          float (&dens)[SPL], float (&gate)[SPL], float (&zz)[SPL],
                                          float (&rgbv)[SPL][3], float& norm, bool* bad_raw = nullptr) {
    const float* rr = c.rays + (long long)ray * 11;
    norm = sqrtf(rr[3] * rr[3] + rr[4] * rr[4] + rr[5] * rr[5]);
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const int j = lane * SPL + e;
        alpha[e] = 0.f; dist[e] = 0.f; dens[e] = 0.f; gate[e] = 0.f; zz[e] = 0.f;
        rgbv[e][0] = rgbv[e][1] = rgbv[e][2] = 0.f;
        if (j < c.S) {
            const long long p = (long long)ray * c.S + j;
            const float4 rw = *reinterpret_cast<const float4*>(c.raw + p * 4);
            if (bad_raw)     // NaN or Inf in the network output (models/lushnerf.py:474-478 checks ret['raw'])
                *bad_raw |= !(fabsf(rw.x) <= 3.402823466e38f) || !(fabsf(rw.y) <= 3.402823466e38f) ||
                            !(fabsf(rw.z) <= 3.402823466e38f) || !(fabsf(rw.w) <= 3.402823466e38f);
            zz[e] = c.z[p];
            rgbv[e][0] = 1.f / (1.f + expf(-rw.x));
            rgbv[e][1] = 1.f / (1.f + expf(-rw.y));
            rgbv[e][2] = 1.f / (1.f + expf(-rw.z));
            if (j < c.S - 1) {
                const float znext = c.z[p + 1];
                dist[e] = (znext - zz[e]) * norm;
                const float pre = comp_pre(rw.w, c.noise, c.noise_std, ray, c.S, j);
                const bool open = comp_gate(pre, znext, c.near_mask);
                dens[e] = open ? fmaxf(pre, 0.f) : 0.f; gate[e] = open ? 1.f : 0.f;
                alpha[e] = 1.f - expf(-dens[e] * dist[e]);
            } else {
                alpha[e] = 1.f;   // last sample: models/lushnerf.py:338
            }
        }
    }
}

// transmittance T_j = prod_{k<j} (1 - alpha_k)
template <int SPL>
__device__ __forceinline__ void comp_trans(const float (&alpha)[SPL], int lane, float (&T)[SPL]) {
    float loc = 1.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) { T[e] = loc; loc *= (1.f - alpha[e]); }
    float incl = wave_incl_prod(loc, lane);
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) T[e] *= excl;
}

}  // namespace lush
