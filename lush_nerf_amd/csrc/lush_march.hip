// lush-march: the ray march proper (z grid, compositing, hierarchical sampling, live-point lists, d rays from d points) + its
// C ABI, and the library's error store.  The ray prologue is lush_rays.hip, the blur kernel lush_rbk.hip, the image tail
// lush_image.hip, draws and Adam lush_step.hip.
// One wavefront (64 lanes) owns one ray: 64 coarse samples map 1:1 onto lanes and
// scans/reductions along the ray are wave-level shuffles.
#include "lush_common.h"
#include "lush_host.h"
#include "lush_composite.h"
#include "../../include/lush_march.h"
#include "../../include/lush_live_fwd.h"

#include <cmath>
#include <string>

namespace lush {

static thread_local std::string g_err;
int set_error(const char* msg) { g_err = msg; return -1; }
int set_hip_error(hipError_t e, const char* what, const char* file, int line) {
    g_err = std::string(hipGetErrorString(e)) + " in " + what + " at " + file + ":" + std::to_string(line);
    return -2;
}

// torch.linspace(0, 1, n)[i] as ATen computes it in fp32
// (aten/src/ATen/native/RangeFactories: step=(end-start)/(n-1); first half counts
// up from start, second half counts down from end).
__device__ __forceinline__ float linspace01(int i, int n) {
    if (n == 1) return 0.f;
    const float step = 1.0f / (float)(n - 1);
    // the count-down half is one fused multiply-add in ATen's vectorised kernel (verified bit-exact
    // against torch.linspace for n = 2..256)
    return i < n / 2 ? __fmul_rn(step, (float)i) : __fmaf_rn(-step, (float)(n - 1 - i), 1.0f);
}

__device__ __forceinline__ float zgrid_at(float near, float far, int i, int S, int lindisp) {
    const float t = linspace01(i, S);
    if (!lindisp) return __fadd_rn(__fmul_rn(near, __fsub_rn(1.f, t)), __fmul_rn(far, t));
    return 1.f / __fadd_rn(__fmul_rn(1.f / near, __fsub_rn(1.f, t)), __fmul_rn(1.f / far, t));
}

// --------------------------------------------------------------------- z grid
__global__ void zgrid_kernel(const float* __restrict__ rays, int R, int S, int lindisp,
                             const float* __restrict__ t_rand, float* __restrict__ z) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)R * S) return;
    const int ray = (int)(i / S), s = (int)(i % S);
    const float near = rays[ray * 11 + 6], far = rays[ray * 11 + 7];
    const float zc = zgrid_at(near, far, s, S, lindisp);
    if (t_rand == nullptr) { z[i] = zc; return; }
    const float zl = s > 0 ? zgrid_at(near, far, s - 1, S, lindisp) : zc;
    const float zr = s < S - 1 ? zgrid_at(near, far, s + 1, S, lindisp) : zc;
    const float lower = s > 0 ? __fmul_rn(.5f, __fadd_rn(zc, zl)) : zc;
    const float upper = s < S - 1 ? __fmul_rn(.5f, __fadd_rn(zr, zc)) : zc;
    z[i] = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), t_rand[i]));
}

__global__ void zfixed_kernel(const float* __restrict__ rays, int R, int S, int index, int lindisp,
                              float* __restrict__ z) {
    const int ray = blockIdx.x * blockDim.x + threadIdx.x;
    if (ray < R) z[ray] = zgrid_at(rays[ray * 11 + 6], rays[ray * 11 + 7], index, S, lindisp);
}

// ---------------------------------------------------------------- compositing (loads and transmittance: lush_composite.h)
template <int SPL>
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void composite_fwd_kernel(CompIn c, float* __restrict__ rgb,
        float* __restrict__ depth, float* __restrict__ acc, float* __restrict__ weights, float* __restrict__ density,
        int* __restrict__ flags, int flag_shift) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= c.R) return;
    float alpha[SPL], dist[SPL], dens[SPL], gate[SPL], zz[SPL], col[SPL][3], T[SPL], norm;
    bool bad_dens = false, bad_raw = false;
    comp_load<SPL>(c, ray, lane, alpha, dist, dens, gate, zz, col, norm, flags != nullptr ? &bad_raw : nullptr);
    comp_trans<SPL>(alpha, lane, T);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, sd = 0.f, sa = 0.f;
#pragma unroll
    for (int e = 0; e < SPL; ++e) {
        const int j = lane * SPL + e;
        const float wgt = alpha[e] * T[e];
        if (j < c.S) {
            if (weights) weights[(long long)ray * c.S + j] = wgt;
            if (density && j < c.S - 1) density[(long long)ray * (c.S - 1) + j] = dens[e];
            if (j < c.S - 1) bad_dens |= !(fabsf(dens[e]) <= 3.402823466e38f);
        }
        s0 += wgt * col[e][0]; s1 += wgt * col[e][1]; s2 += wgt * col[e][2];
        sd += wgt * zz[e]; sa += wgt;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); sd = wave_sum(sd); sa = wave_sum(sa);
    if (flags != nullptr) {   // wave-uniform branch; the ballots run with all lanes active
        const bool any_dens = __ballot(bad_dens) != 0ull, any_raw = __ballot(bad_raw) != 0ull;
        if (lane == 0) {
            if (c.white_bkgd) { s0 += 1.f - sa; s1 += 1.f - sa; s2 += 1.f - sa; }
            auto bad = [](float v) { return !(fabsf(v) <= 3.402823466e38f); };      // NaN or Inf
            const int w = (bad(s0) || bad(s1) || bad(s2) ? LUSH_FAULT_RGB : 0) | (bad(sd) ? LUSH_FAULT_DEPTH : 0) |
                          (bad(sa) ? LUSH_FAULT_ACC : 0) | (any_dens ? LUSH_FAULT_DENSITY : 0) | (any_raw ? LUSH_FAULT_RAW : 0);
            if (w) atomicOr(flags, w << flag_shift);
            rgb[ray * 3 + 0] = s0; rgb[ray * 3 + 1] = s1; rgb[ray * 3 + 2] = s2;
            depth[ray] = sd; acc[ray] = sa;
        }
        return;
    }
    if (lane == 0) {
        if (c.white_bkgd) { s0 += 1.f - sa; s1 += 1.f - sa; s2 += 1.f - sa; }
        rgb[ray * 3 + 0] = s0; rgb[ray * 3 + 1] = s1; rgb[ray * 3 + 2] = s2;
        depth[ray] = sd; acc[ray] = sa;
    }
}

// What the backward of a pass needs besides d_raw, folded into this kernel so that it costs no launch of its own (round 4):
//   block_max  per-workgroup max |d_raw| (one float per workgroup of this launch, plain stores), or NULL: loss_scale_kernel turns
//            them into the fp16 gradient chain's loss scale.  (A first version ended in the "last workgroup to finish" pattern
//            of grad_scale_kernel: 2 x 2048 atomics on one word took this kernel from 27 to 127 us.)
//   zero_buf a scratch the weight-gradient launch accumulates into (the feature-factor block), zeroed here, or NULL;
//   init_drays: drays is written whole (zeros outside columns 3..5) instead of added to -- the first pass of a march.
struct CompBwdExtra { float* block_max; float* zero_buf; long long zero_n; int init_drays; };

template <int SPL>
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void composite_bwd_kernel(CompIn c, const float* __restrict__ g_rgb,
        const float* __restrict__ g_depth, const float* __restrict__ g_acc, float* __restrict__ draw,
        float* __restrict__ drays, CompBwdExtra X) {
    const int lane = threadIdx.x & 63;
    if (X.zero_buf != nullptr)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < X.zero_n; i += (long long)gridDim.x * blockDim.x) X.zero_buf[i] = 0.f;
    float vmax = 0.f;
  for (int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6); ray < c.R; ray += gridDim.x * RAYS_PER_BLOCK) {
    float alpha[SPL], dist[SPL], dens[SPL], gate[SPL], zz[SPL], col[SPL][3], T[SPL], norm;
    comp_load<SPL>(c, ray, lane, alpha, dist, dens, gate, zz, col, norm);
    comp_trans<SPL>(alpha, lane, T);
    float gr[3] = {0.f, 0.f, 0.f};
    if (g_rgb) { gr[0] = g_rgb[ray * 3]; gr[1] = g_rgb[ray * 3 + 1]; gr[2] = g_rgb[ray * 3 + 2]; }
    const float gd = g_depth ? g_depth[ray] : 0.f;
    float ga = g_acc ? g_acc[ray] : 0.f;
    if (c.white_bkgd) ga -= gr[0] + gr[1] + gr[2];
    // G_j = dL/dw_j ; S_j = sum_{k>j} G_k alpha_k prod_{j<m<k}(1-alpha_m): reverse scan of the
    // affine maps f_k(s) = G_k alpha_k + (1-alpha_k) s, composed (a1,b1)o(a2,b2) = (a1 a2, a1 b2 + b1).
    float G[SPL];
#pragma unroll
    for (int e = 0; e < SPL; ++e) G[e] = gr[0] * col[e][0] + gr[1] * col[e][1] + gr[2] * col[e][2] + gd * zz[e] + ga;
    // lane aggregate F = f_{first} o ... o f_{last} of this lane's samples
    float Fa = 1.f, Fb = 0.f;
#pragma unroll
    for (int e = SPL - 1; e >= 0; --e) {   // F <- f_e o F
        Fb = G[e] * alpha[e] + (1.f - alpha[e]) * Fb;
        Fa = (1.f - alpha[e]) * Fa;
    }
    // suffix composition over lanes: Suf_l = F_l o F_{l+1} o ... o F_63
    float Sa = Fa, Sb = Fb;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ta = __shfl_down(Sa, o, 64), tb = __shfl_down(Sb, o, 64);
        if (lane + o < 64) { Sb = Sa * tb + Sb; Sa = Sa * ta; }
    }
    float tail = __shfl_down(Sb, 1, 64);   // value of everything after this lane, applied to 0
    if (lane == 63) tail = 0.f;
    float dnorm = 0.f;
    float sfx = tail;                        // S_j for the lane's last sample
#pragma unroll
    for (int e = SPL - 1; e >= 0; --e) {
        const int j = lane * SPL + e;
        const float wgt = alpha[e] * T[e];
        float4 o = {0.f, 0.f, 0.f, 0.f};
        if (j < c.S) {
            o.x = wgt * gr[0] * col[e][0] * (1.f - col[e][0]);
            o.y = wgt * gr[1] * col[e][1] * (1.f - col[e][1]);
            o.z = wgt * gr[2] * col[e][2] * (1.f - col[e][2]);
            if (j < c.S - 1) {
                const float dalpha = T[e] * (G[e] - sfx);
                const float om = 1.f - alpha[e];            // = exp(-dens*dist)
                o.w = dalpha * dist[e] * om * gate[e];
                const float ddist = dalpha * dens[e] * om;
                dnorm += ddist * (dist[e] / (norm > 0.f ? norm : 1.f));
            }
            *reinterpret_cast<float4*>(draw + ((long long)ray * c.S + j) * 4) = o;
            vmax = fmaxf(fmaxf(vmax, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
        }
        sfx = G[e] * alpha[e] + (1.f - alpha[e]) * sfx;     // becomes S_{j-1}
    }
    dnorm = wave_sum(dnorm);
    if (drays != nullptr) {     // (the passes of a march run one after the other on one stream)
        if (X.init_drays) {
            if (lane < 11) drays[(long long)ray * 11 + lane] = (lane >= 3 && lane < 6 && norm > 0.f) ? dnorm * c.rays[(long long)ray * 11 + lane] / norm : 0.f;
        } else if (lane < 3 && norm > 0.f) {
            drays[(long long)ray * 11 + 3 + lane] += dnorm * c.rays[(long long)ray * 11 + 3 + lane] / norm;
        }
    }
  }
    if (X.block_max != nullptr) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o, 64));
        __shared__ float sm[RAYS_PER_BLOCK];
        if (lane == 0) sm[threadIdx.x >> 6] = vmax;
        __syncthreads();
        if (threadIdx.x == 0) {
            float m = 0.f;
#pragma unroll
            for (int i = 0; i < RAYS_PER_BLOCK; ++i) m = fmaxf(m, sm[i]);
            X.block_max[blockIdx.x] = m;
        }
    }
}

// {scale, 1/scale} of the loss-scaled fp16 gradient chain from n per-workgroup maxima of |d_raw|: the power of two that puts
// the maximum into [8, 16); 1 when d_raw is all zero or not finite (grad_scale_kernel's rule).  One workgroup.
__global__ __launch_bounds__(256) void loss_scale_kernel(const float* __restrict__ block_max, int n, float* __restrict__ scale2) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = block_max[i];
        m = (v <= 3.402823466e38f) ? fmaxf(m, v) : __int_as_float(0x7f800000);      // (Inf stays Inf; NaN cannot come out of fmaxf)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
        loss_scale_rule(mx, scale2);
    }
}

// ------------------------------------------------------ hierarchical sampling
constexpr int SM_MAXN = 512;   // S + Ni rounded up to a power of two

// Bitonic sort of 64 * EPL values held EPL per lane, element e * 64 + lane in v[e], ascending: the same network as the LDS
// form below (so the same result: a sorting network's output is the sorted sequence), but a compare-exchange across lanes is one
// cross-lane read and a min / max instead of two LDS reads, two conditional LDS writes and a wait, partners 64 or more apart are
// registers of the same lane, and everything is unrolled (the LDS form's 28-64 steps ran ~40 instructions each for two elements).
template <int EPL>
__device__ __forceinline__ void wave_bitonic_sort(float (&v)[EPL], int lane) {
#pragma unroll
    for (int k = 2; k <= 64 * EPL; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    if ((e & (j >> 6)) == 0) {
                        const int pe = e | (j >> 6);
                        const bool up = ((e * 64) & k) == 0;          // (k >= 128 here: the direction depends on e only)
                        const float lo = fminf(v[e], v[pe]), hi = fmaxf(v[e], v[pe]);
                        v[e] = up ? lo : hi;
                        v[pe] = up ? hi : lo;
                    }
                }
            } else {
                const bool lower = (lane & j) == 0;
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const float o = __shfl_xor(v[e], j, 64);
                    const bool up = ((e * 64 + lane) & k) == 0;
                    v[e] = (lower == up) ? fminf(v[e], o) : fmaxf(v[e], o);
                }
            }
        }
    }
}
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void sample_merge_kernel(const float* __restrict__ z,
        const float* __restrict__ weights, int R, int S, int Ni, const float* __restrict__ u,
        float* __restrict__ z_out, float* __restrict__ z_samples, float* __restrict__ z_std, int* __restrict__ flags) {
    __shared__ float s_cdf[RAYS_PER_BLOCK][256];
    __shared__ float s_bins[RAYS_PER_BLOCK][256];
    __shared__ float s_sort[RAYS_PER_BLOCK][SM_MAXN];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + wv;
    if (ray >= R) return;                   // whole wave exits together
    float* cdf = s_cdf[wv];
    float* bins = s_bins[wv];
    float* srt = s_sort[wv];
    const float* zr = z + (long long)ray * S;
    const float* wr = weights + (long long)ray * S;
    const int nb = S - 1;                   // knots in cdf and entries in bins
    // pdf over weights[1..S-2] + 1e-5, inclusive scan in chunks of 64
    float tot = 0.f;
    for (int k = lane; k < S - 2; k += 64) tot += wr[k + 1] + 1e-5f;
    tot = wave_sum(tot);
    float carry = 0.f;
    if (lane == 0) cdf[0] = 0.f;
    for (int k0 = 0; k0 < S - 2; k0 += 64) {
        const int k = k0 + lane;
        const float pdf = k < S - 2 ? (wr[k + 1] + 1e-5f) / tot : 0.f;
        const float inc = wave_incl_sum(pdf, lane) + carry;
        if (k < S - 2) cdf[k + 1] = inc;
        carry = __shfl(inc, 63, 64);
    }
    for (int k = lane; k < nb; k += 64) bins[k] = .5f * (zr[k + 1] + zr[k]);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);    // lgkmcnt(0): LDS writes visible to the wave
    // inverse CDF
    float sum = 0.f;
    const int N = S + Ni;
    // whole 64-value rows of coarse depths and of new samples: the union is sorted in registers (wave_bitonic_sort)
    // (a lane keeps four rows of new samples: more than 256 of them take the LDS network below)
    const bool in_regs = (S & 63) == 0 && (Ni & 63) == 0 && Ni <= 256;
    float smp_r[4] = {0.f, 0.f, 0.f, 0.f};            // sample lane + 64 t
    int t_idx = 0;
    for (int i = lane; i < Ni; i += 64, ++t_idx) {
        const float uu = u ? u[(long long)ray * Ni + i] : linspace01(i, Ni);
        int lo = 0, hi = nb;                // first index with cdf > uu  (searchsorted right=True)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] <= uu) lo = mid + 1; else hi = mid;
        }
        const int below = lo - 1 > 0 ? lo - 1 : 0;
        const int above = lo < nb - 1 ? lo : nb - 1;
        const float cb = cdf[below], ca = cdf[above];
        float denom = ca - cb;
        if (denom < 1e-5f) denom = 1.f;
        const float t = (uu - cb) / denom;
        const float bb = bins[below];
        const float smp = bb + t * (bins[above] - bb);
        if (z_samples) z_samples[(long long)ray * Ni + i] = smp;
        srt[S + i] = smp;
        if (t_idx == 0) smp_r[0] = smp; else if (t_idx == 1) smp_r[1] = smp; else if (t_idx == 2) smp_r[2] = smp; else if (t_idx == 3) smp_r[3] = smp;
        sum += smp;
    }
    sum = wave_sum(sum);
    const float mean = sum / (float)Ni;
    float var = 0.f;
    for (int i = lane; i < Ni; i += 64) { const float d = srt[S + i] - mean; var += d * d; }
    var = wave_sum(var);
    if (lane == 0) {
        const float sd = sqrtf(var / (float)Ni);
        if (z_std) z_std[ray] = sd;
        if (flags != nullptr && !(fabsf(sd) <= 3.402823466e38f)) atomicOr(flags, LUSH_FAULT_ZSTD);
    }
    // sort(cat(z, samples)): bitonic network over N2 >= N values padded with +inf
    int N2 = 64;
    while (N2 < N) N2 <<= 1;
    if (in_regs && N2 >= 128) {
        const int sr = S >> 6, nr = Ni >> 6;           // rows of depths, rows of samples
        auto sorted_rows = [&](auto epl_c) {
            constexpr int EPL = decltype(epl_c)::value;
            float v[EPL];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                float x = __builtin_inff();
                if (e < sr) x = zr[e * 64 + lane];
                else if (e - sr < nr) x = (e - sr) == 0 ? smp_r[0] : (e - sr) == 1 ? smp_r[1] : (e - sr) == 2 ? smp_r[2] : smp_r[3];
                v[e] = x;
            }
            wave_bitonic_sort<EPL>(v, lane);
#pragma unroll
            for (int e = 0; e < EPL; ++e)
                if (e * 64 < N) z_out[(long long)ray * N + e * 64 + lane] = v[e];      // (N is a multiple of 64 here)
        };
        if (N2 == 128) sorted_rows(std::integral_constant<int, 2>{});
        else if (N2 == 256) sorted_rows(std::integral_constant<int, 4>{});
        else sorted_rows(std::integral_constant<int, 8>{});
        return;
    }
    for (int i = lane; i < S; i += 64) srt[i] = zr[i];
    for (int i = N + lane; i < N2; i += 64) srt[i] = __builtin_inff();
    __builtin_amdgcn_wave_barrier();
    for (int k = 2; k <= N2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < N2; i += 64) {
                const int p = i ^ j;
                if (p > i) {
                    const float a = srt[i], b = srt[p];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { srt[i] = b; srt[p] = a; }
                }
            }
        }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < N; i += 64) z_out[(long long)ray * N + i] = srt[i];
}

// ------------------------------------------------------- d rays from d points
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void ray_grad_reduce_kernel(const float* __restrict__ dpts,
        const float* __restrict__ z, int R, int S, float* __restrict__ drays) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= R) return;
    float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // (up to 256 samples with every load in flight before the first is used: as a loop with a run-time trip count each 64
    // samples waited for their own three loads; more samples take the loop)
    for (int s0 = 0; s0 < S; s0 += 256) {
        float4 gx[4], gv[4];
        float zz[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int s = s0 + c * 64 + lane;
            const bool in = s < S;
            const long long p = (long long)ray * S + (in ? s : 0);
            gx[c] = *reinterpret_cast<const float4*>(dpts + p * 8);
            gv[c] = *reinterpret_cast<const float4*>(dpts + p * 8 + 4);
            zz[c] = z[p];
            if (!in) { gx[c] = make_float4(0.f, 0.f, 0.f, 0.f); gv[c] = gx[c]; }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {          // (chunks in order: the order of the sums is the loop's)
            if (s0 + c * 64 < S) {
                a[0] += gx[c].x; a[1] += gx[c].y; a[2] += gx[c].z;
                a[3] += gx[c].x * zz[c]; a[4] += gx[c].y * zz[c]; a[5] += gx[c].z * zz[c];
                a[6] += gv[c].x; a[7] += gv[c].y; a[8] += gv[c].z;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = wave_sum(a[i]);
    // one addition per word by lanes 0..8 (a read-modify-write by lane 0 waited for its own nine loads; this ray's words are
    // touched by no other wave of the launch, and the launches of a step run one after the other)
    float mine = a[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) mine = lane == i ? a[i] : mine;
    if (lane < 9) atomicAdd(drays + (long long)ray * 11 + (lane < 6 ? lane : lane + 2), mine);
}

// ------------------------------------------------------- live points (round 5)
// A sample whose density pre-activation is clamped by the ReLU of raw2outputs (models/lushnerf.py:313: relu(raw + noise)) has
// alpha = 0, weight = 0 and d alpha / d raw = 0: its d_raw row is EXACTLY zero and nothing flows back through its MLP
// evaluation.  With raw_noise_std = 1 (every shipped config) and a density near zero that is half of all the points.  The
// backward therefore runs on the LIVE points only: this compaction lists them (in grid order: deterministic), gathers their
// d_raw rows and gives every ray its range of the list; the forward is re-run with the stash on that list, the gradient
// chain and the weight gradients see a dense launch of `cnt` points.  Sums skip exact zeros only: same gradients.
constexpr int LIVE_BLK = 1024;
__device__ __forceinline__ bool live_row(const float4 v) { return v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f; }      // (NaN counts as live)

// What decides that a point is listed, and what travels with a listed point.  LiveByDraw: the backward's list (a non-zero d_raw
// row, gathered into draw_c, zero rows behind the list).  LiveByAlpha: the forward's list of a march in the trunk-only form
// (include/lush_live_fwd.h) -- the points the compositing gives a non-zero alpha: comp_gate(), and the last sample of a ray,
// whose alpha is 1 (comp_load).
struct LiveByDraw {
    const float4* draw; float4* draw_c;
    __device__ __forceinline__ bool live(int p, float4& v) const { v = draw[p]; return live_row(v); }
    __device__ __forceinline__ void emit(int pos, const float4& v) const { draw_c[pos] = v; }
    __device__ __forceinline__ void pad(int p) const { draw_c[p] = make_float4(0.f, 0.f, 0.f, 0.f); }
};
struct LiveByAlpha {
    const float *raw, *z, *noise; float noise_std, near_mask; int S;
    __device__ __forceinline__ bool live(int p, float4&) const {
        const int ray = p / S, j = p - ray * S;
        if (j == S - 1) return true;
        return comp_gate(comp_pre(raw[(long long)p * 4 + 3], noise, noise_std, ray, S, j), z[p + 1], near_mask);
    }
    __device__ __forceinline__ void emit(int, const float4&) const {}
    __device__ __forceinline__ void pad(int) const {}
};

template <class Pred>
__global__ __launch_bounds__(256) void live_count_kernel(const Pred pred, int P, int* __restrict__ blk) {
    const int p0 = blockIdx.x * LIVE_BLK + threadIdx.x * 4;
    int c = 0;
    float4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (p0 + k < P) c += pred.live(p0 + k, v) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}
// one workgroup: exclusive scan of the block counts in place; cnt[0] = the number of live points, cnt[1] = P
__global__ __launch_bounds__(1024) void live_scan_kernel(int* __restrict__ blk, int nblk, int P, int* __restrict__ cnt) {
    __shared__ int sm[1024];
    int carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int i = b0 + (int)threadIdx.x;
        const int v = i < nblk ? blk[i] : 0;
        sm[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int a = (int)threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
            __syncthreads();
            sm[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nblk) blk[i] = carry + sm[threadIdx.x] - v;
        const int tot = sm[1023];
        __syncthreads();
        carry += tot;
    }
    if (threadIdx.x == 0) { cnt[0] = carry; cnt[1] = P; }
}
template <class Pred>
__global__ __launch_bounds__(256) void live_scatter_kernel(const Pred pred, int P, int S, int R, const int* __restrict__ blk_off,
                                                          const int* __restrict__ cnt, int* __restrict__ live_idx, int* __restrict__ ray_start) {
    const int p0 = blockIdx.x * LIVE_BLK + threadIdx.x * 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 v[4];
    int f[4], c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        f[k] = (p0 + k < P && pred.live(p0 + k, v[k])) ? 1 : 0;
        c += f[k];
    }
    int incl = c;                                   // inclusive scan over the workgroup's 256 threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int a = __shfl_up(incl, o, 64); if (lane >= o) incl += a; }
    __shared__ int sm[4];
    if (lane == 63) sm[w] = incl;
    __syncthreads();
    int base = blk_off[blockIdx.x];
    for (int i = 0; i < w; ++i) base += sm[i];
    int pos = base + incl - c;
    const int total = cnt[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k;
        if (p < P) {
            if (p % S == 0) ray_start[p / S] = pos;          // where ray p / S begins in the list
            if (f[k]) { live_idx[pos] = p; pred.emit(pos, v[k]); ++pos; }
            if (p >= total) pred.pad(p);      // rows behind the list: zero (tile padding, the loss scale's pass)
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ray_start[R] = total;
}

// d_raw rows of a list made before they existed (the forward's, LiveByAlpha) in list order: draw_c[i] = draw[live_idx[i]], zero
// rows behind the list as LiveByDraw::pad leaves them; cnt[0] (zeroed by the caller) counts the non-zero rows, cnt[1] = P
__global__ __launch_bounds__(256) void live_gather_kernel(const float4* __restrict__ draw, int P, const int* __restrict__ live_idx,
                                                         const int* __restrict__ list_cnt, float4* __restrict__ draw_c, int* __restrict__ cnt) {
    const int n = list_cnt[0];
    int c = 0;
#pragma unroll
    for (int k = 0; k < LIVE_BLK / 256; ++k) {
        const int i = blockIdx.x * LIVE_BLK + k * 256 + threadIdx.x;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n && i < P) v = draw[live_idx[i]];
        if (i < P) draw_c[i] = v;
        c += live_row(v) ? 1 : 0;
    }
    // ONE addition per workgroup (an integer sum: the order does not show): one per wave, all to the same word, took 0.24 ms of
    // the headline step's 2.6 M rows
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ int sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = sm[0] + sm[1] + sm[2] + sm[3];
        if (t) atomicAdd(cnt, t);
        if (blockIdx.x == 0) cnt[1] = P;
    }
}

// d rays from the d(point) rows of a live-point launch: ray r owns rows [ray_start[r], ray_start[r + 1]) of the list
__global__ __launch_bounds__(RAYS_PER_BLOCK * 64) void ray_grad_reduce_live_kernel(const float* __restrict__ dpts, const float* __restrict__ z,
        const int* __restrict__ live_idx, const int* __restrict__ ray_start, int R, float* __restrict__ drays) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= R) return;
    const int b = ray_start[ray], e = ray_start[ray + 1];
    float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = b + lane; i < e; i += 64) {
        const float4 gx = *reinterpret_cast<const float4*>(dpts + (long long)i * 8);
        const float4 gv = *reinterpret_cast<const float4*>(dpts + (long long)i * 8 + 4);
        const float zz = z[live_idx[i]];
        a[0] += gx.x; a[1] += gx.y; a[2] += gx.z;
        a[3] += gx.x * zz; a[4] += gx.y * zz; a[5] += gx.z * zz;
        a[6] += gv.x; a[7] += gv.y; a[8] += gv.z;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = wave_sum(a[i]);
    float mine = a[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) mine = lane == i ? a[i] : mine;
    if (lane < 9) atomicAdd(drays + (long long)ray * 11 + (lane < 6 ? lane : lane + 2), mine);
}

}  // namespace lush

// =============================================================================
// C ABI
// =============================================================================
using namespace lush;

// count, scan, scatter: the list of the points `pred` calls live, in grid order (lush_live_compact, lush_live_list)
template <class Pred>
static int live_list(const Pred& pred, long long P, int R, int S, int* live_idx, int* ray_start, int* cnt, int* blk, lush_stream_t st) {
    const int nblk = (int)((P + LIVE_BLK - 1) / LIVE_BLK);
    if (int rc = launch(live_count_kernel<Pred>, dim3(nblk), dim3(256), 0, st, pred, (int)P, blk)) return rc;
    if (int rc = launch(live_scan_kernel, dim3(1), dim3(1024), 0, st, blk, nblk, (int)P, cnt)) return rc;
    return launch(live_scatter_kernel<Pred>, dim3(nblk), dim3(256), 0, st, pred, (int)P, S, R, blk, cnt, live_idx, ray_start);
}

extern "C" {

const char* lush_last_error(void) { return g_err.c_str(); }
int lush_abi_version(void) { return LUSH_ABI_VERSION; }

int lush_zgrid(const float* rays, int R, int S, int lindisp, const float* t_rand, float* z, lush_stream_t st) {
    if (R <= 0 || S <= 0) return set_error("lush_zgrid: empty");
    return launch(zgrid_kernel, dim3(cdiv((long long)R * S, 256)), dim3(256), 0, st, rays, R, S, lindisp, t_rand, z);
}
int lush_zfixed(const float* rays, int R, int S, int index, int lindisp, float* z, lush_stream_t st) {
    if (index < 0 || index >= S) return set_error("lush_zfixed: index out of range");
    return launch(zfixed_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, rays, R, S, index, lindisp, z);
}

int lush_composite_fwd(const float* raw, const float* z, const float* rays, int R, int S, const float* noise,
                       float noise_std, float near_mask, int white_bkgd, float* rgb, float* depth, float* acc,
                       float* weights, float* density, int* flags, int flag_shift, lush_stream_t st) {
    if (S < 2 || S > 256) return set_error("lush_composite_fwd: S must be in [2,256]");
    if (flag_shift < 0 || flag_shift > 16) return set_error("lush_composite_fwd: flag_shift must be in [0,16]");
    CompIn c{raw, z, rays, noise, R, S, noise_std, near_mask, white_bkgd};
    dim3 g(cdiv(R, RAYS_PER_BLOCK)), b(RAYS_PER_BLOCK * 64);
    return comp_for_spl(S, [&](auto spl) {
        return launch(composite_fwd_kernel<decltype(spl)::value>, g, b, 0, st, c, rgb, depth, acc, weights, density, flags, flag_shift); });
}
static int composite_bwd_blocks(int R) {
    // at most 2048 workgroups (8 per CU: what is resident at once) walk the rays
    int blocks = cdiv(R, RAYS_PER_BLOCK);
    return blocks > 2048 ? 2048 : blocks;
}
int lush_composite_bwd_blocks(int R) { return R > 0 ? composite_bwd_blocks(R) : 0; }

int lush_composite_bwd(const float* raw, const float* z, const float* rays, int R, int S, const float* noise,
                       float noise_std, float near_mask, int white_bkgd, const float* g_rgb, const float* g_depth,
                       const float* g_acc, float* draw, float* drays, float* block_max, float* zero_buf, long long zero_n,
                       int init_drays, lush_stream_t st) {
    if (S < 2 || S > 256) return set_error("lush_composite_bwd: S must be in [2,256]");
    if (zero_buf != nullptr && zero_n < 0) return set_error("lush_composite_bwd: zero_n must not be negative");
    CompIn c{raw, z, rays, noise, R, S, noise_std, near_mask, white_bkgd};
    const CompBwdExtra x{block_max, zero_buf, zero_buf ? zero_n : 0, init_drays};
    dim3 g(composite_bwd_blocks(R)), b(RAYS_PER_BLOCK * 64);
    return comp_for_spl(S, [&](auto spl) {
        return launch(composite_bwd_kernel<decltype(spl)::value>, g, b, 0, st, c, g_rgb, g_depth, g_acc, draw, drays, x); });
}
int lush_loss_scale(const float* block_max, int n, float* scale2, lush_stream_t st) {
    if (!block_max || n < 1 || !scale2) return set_error("lush_loss_scale: maxima and destination are required");
    return launch(loss_scale_kernel, dim3(1), dim3(256), 0, st, block_max, n, scale2);
}

int lush_sample_merge(const float* z, const float* weights, int R, int S, int Ni, const float* u, float* z_out,
                      float* z_samples, float* z_std, int* flags, lush_stream_t st) {
    if (S < 3 || S > 256 || Ni < 1 || S + Ni > SM_MAXN) return set_error("lush_sample_merge: need 3<=S<=256, S+Ni<=512");
    return launch(sample_merge_kernel, dim3(cdiv(R, RAYS_PER_BLOCK)), dim3(RAYS_PER_BLOCK * 64), 0, st, z, weights, R, S, Ni, u, z_out,
                  z_samples, z_std, flags);
}

int lush_ray_grad_reduce(const float* dpts, const float* z, int R, int S, float* drays, lush_stream_t st) {
    return launch(ray_grad_reduce_kernel, dim3(cdiv(R, RAYS_PER_BLOCK)), dim3(RAYS_PER_BLOCK * 64), 0, st, dpts, z, R, S, drays);
}

size_t lush_live_aux_bytes(long long P) { return P > 0 ? (size_t)((P + LIVE_BLK - 1) / LIVE_BLK) * sizeof(int) : 0; }

int lush_live_compact(const float* draw, int R, int S, int* live_idx, float* draw_c, int* ray_start, int* cnt, void* aux, lush_stream_t st) {
    const long long P = (long long)R * S;
    if (R <= 0 || S <= 0 || P >= (1LL << 27)) return set_error("lush_live_compact: 1 .. 2^27 - 1 points");
    if (!draw || !live_idx || !draw_c || !ray_start || !cnt || !aux) return set_error("lush_live_compact: every buffer is required");
    return live_list(LiveByDraw{(const float4*)draw, (float4*)draw_c}, P, R, S, live_idx, ray_start, cnt, (int*)aux, st);
}

int lush_live_list(const float* raw, const float* z, const float* noise, float noise_std, float near_mask, int R, int S,
                   int* live_idx, int* ray_start, int* cnt, void* aux, lush_stream_t st) {
    const long long P = (long long)R * S;
    if (R <= 0 || S <= 0 || P >= (1LL << 27)) return set_error("lush_live_list: 1 .. 2^27 - 1 points");
    if (!raw || !z || !live_idx || !ray_start || !cnt || !aux) return set_error("lush_live_list: raw, z and every output buffer are required");
    return live_list(LiveByAlpha{raw, z, noise, noise_std, near_mask, S}, P, R, S, live_idx, ray_start, cnt, (int*)aux, st);
}

int lush_live_gather(const float* draw, int R, int S, const int* live_idx, const int* list_cnt, float* draw_c, int* cnt, lush_stream_t st) {
    const long long P = (long long)R * S;
    if (R <= 0 || S <= 0 || P >= (1LL << 27)) return set_error("lush_live_gather: 1 .. 2^27 - 1 points");
    if (!draw || !live_idx || !list_cnt || !draw_c || !cnt) return set_error("lush_live_gather: every buffer is required");
    if (hipMemsetAsync(cnt, 0, sizeof(int), (hipStream_t)st) != hipSuccess) return set_error("lush_live_gather: hipMemsetAsync failed");
    return launch(live_gather_kernel, dim3(cdiv(P, LIVE_BLK)), dim3(256), 0, st, (const float4*)draw, (int)P, live_idx, list_cnt, (float4*)draw_c, cnt);
}

int lush_ray_grad_reduce_live(const float* dpts, const float* z, const int* live_idx, const int* ray_start, int R, float* drays, lush_stream_t st) {
    return launch(ray_grad_reduce_live_kernel, dim3(cdiv(R, RAYS_PER_BLOCK)), dim3(RAYS_PER_BLOCK * 64), 0, st, dpts, z, live_idx, ray_start, R, drays);
}

}  // extern "C"
