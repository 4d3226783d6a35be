// lush-march: the image tail + its C ABI -- what NeRFAll.forward does with rendered colours (models/lushnerf.py:644-654: the
// blur kernel's weighted sum, the noise activation, tone mapping), the training loss and the consistency loss
// (run_lushnerf.py:644-650).
#include "lush_common.h"
#include "lush_host.h"
#include "../../include/lush_march.h"

namespace lush {

// ------------------------------------------------------- blur mix / tone map
__global__ void wsum_fwd_kernel(const float* __restrict__ x, const float* __restrict__ ccw, int N, int M, int C,
                                float* __restrict__ y) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * C) return;
    const long long n = t / C; const int c = (int)(t % C);
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += x[(n * M + m) * C + c] * ccw[n * M + m];
    y[t] = s;
}
__global__ void wsum_bwd_kernel(const float* __restrict__ x, const float* __restrict__ ccw, int N, int M, int C,
                                const float* __restrict__ dy, float* __restrict__ dx, float* __restrict__ dccw) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (n, m)
    if (t >= (long long)N * M) return;
    const long long n = t / M;
    float s = 0.f;
    const float w = ccw[t];
    for (int c = 0; c < C; ++c) {
        const float g = dy[n * C + c];
        s += g * x[t * C + c];
        if (dx) dx[t * C + c] = g * w;
    }
    if (dccw) dccw[t] = s;
}

constexpr float INV_GAMMA = (float)(1.0 / 2.2);
__device__ __forceinline__ float tm_apply(float v, int gamma) { return gamma ? powf(v, INV_GAMMA) : v; }
__device__ __forceinline__ float tm_slope(float v, int gamma) { return gamma ? INV_GAMMA * powf(v, INV_GAMMA - 1.f) : 1.f; }
__global__ void tonemap_fwd_kernel(const float* __restrict__ x, const float* __restrict__ nraw, int n3, int gamma,
                                   float* __restrict__ y) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    float v = x[t];
    if (nraw) v += 0.1f * (1.f / (1.f + expf(-nraw[t])));
    y[t] = tm_apply(v, gamma);
}
__global__ void tonemap_bwd_kernel(const float* __restrict__ x, const float* __restrict__ nraw, int n3, int gamma,
                                   const float* __restrict__ dy, float* __restrict__ dx, float* __restrict__ dnraw) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n3) return;
    float v = x[t], sg = 0.f;
    if (nraw) { sg = 1.f / (1.f + expf(-nraw[t])); v += 0.1f * sg; }
    // ((dy INV_GAMMA) pow: not dy tm_slope(v), which rounds INV_GAMMA pow first)
    const float gv = gamma ? dy[t] * INV_GAMMA * powf(v, INV_GAMMA - 1.f) : dy[t];
    if (dx) dx[t] = gv;
    if (nraw && dnraw) dnraw[t] = gv * 0.1f * sg * (1.f - sg);
}
__global__ void noise_act_fwd_kernel(const float* __restrict__ x, int n, float* __restrict__ y) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) y[t] = 0.1f * (1.f / (1.f + expf(-x[t])));
}
__global__ void noise_act_bwd_kernel(const float* __restrict__ x, int n, const float* __restrict__ dy,
                                     float* __restrict__ dx) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { const float s = 1.f / (1.f + expf(-x[t])); dx[t] = dy[t] * 0.1f * s * (1.f - s); }
}
// ------------------------------------------------- blur mix + noise + tone map in one (SURVEY 7.2 `blur_mix_tonemap`)
// The tail of NeRFAll.forward's training branch (models/lushnerf.py:644-654): rbk_weighted_sum of the fine and the coarse
// colour (:100-116), rgb_noise = 0.1 sigmoid(noise_raw) (:649), and the five tone-mapped / plain outputs of the 7-tuple
//   blur = tm(sum_m ccw x + rgb_noise), blur0 likewise, noise = rgb_noise, sharp = tm(sum_m ccw x), sharp0 likewise.
// One thread per (input ray, channel); the weighted sums in the order of wsum_fwd_kernel (m ascending).
__global__ void blur_mix_fwd_kernel(const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ ccw,
                                    const float* __restrict__ nraw, int nraw_ld, int N, int M1, int gamma, float* __restrict__ blur,
                                    float* __restrict__ blur0, float* __restrict__ noise, float* __restrict__ sharp,
                                    float* __restrict__ sharp0) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * 3) return;
    const long long n = t / 3;
    const int c = (int)(t % 3);
    float s = 0.f, s0 = 0.f;
    for (int m = 0; m < M1; ++m) {
        const float w = ccw[n * M1 + m];
        s += rgb[(n * M1 + m) * 3 + c] * w;
        s0 += rgb0[(n * M1 + m) * 3 + c] * w;
    }
    const float nz = 0.1f * (1.f / (1.f + expf(-nraw[n * nraw_ld + c])));
    blur[t] = tm_apply(s + nz, gamma);
    blur0[t] = tm_apply(s0 + nz, gamma);
    noise[t] = nz;
    sharp[t] = tm_apply(s, gamma);
    sharp0[t] = tm_apply(s0, gamma);
}
// Reverse: one thread per (input ray, motion slot).  Any of the five output gradients may be NULL (= 0).  d_rgb / d_rgb0
// [N*M1][3], d_ccw [N][M1], d_nraw [N][4] overwritten (d_nraw by the slot-0 thread; column 3 = 0: the row is the noise MLP's
// d_raw as it stands).
__global__ void blur_mix_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ rgb0, const float* __restrict__ ccw,
                                    const float* __restrict__ nraw, int nraw_ld, int N, int M1, int gamma, const float* __restrict__ g_blur,
                                    const float* __restrict__ g_blur0, const float* __restrict__ g_noise,
                                    const float* __restrict__ g_sharp, const float* __restrict__ g_sharp0,
                                    float* __restrict__ d_rgb, float* __restrict__ d_rgb0, float* __restrict__ d_ccw,
                                    float* __restrict__ d_nraw) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * M1) return;
    const long long n = t / M1;
    const int slot = (int)(t % M1);
    const float w = ccw[t];
    float dw = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float s = 0.f, s0 = 0.f;            // (recomputed per thread: M1 * 6 loads that the wave's neighbours share through L1)
        for (int m = 0; m < M1; ++m) {
            const float wm = ccw[n * M1 + m];
            s += rgb[(n * M1 + m) * 3 + c] * wm;
            s0 += rgb0[(n * M1 + m) * 3 + c] * wm;
        }
        const float sg = 1.f / (1.f + expf(-nraw[n * nraw_ld + c]));
        const float nz = 0.1f * sg;
        const float gb = g_blur ? g_blur[n * 3 + c] * tm_slope(s + nz, gamma) : 0.f;
        const float gb0 = g_blur0 ? g_blur0[n * 3 + c] * tm_slope(s0 + nz, gamma) : 0.f;
        const float gs = gb + (g_sharp ? g_sharp[n * 3 + c] * tm_slope(s, gamma) : 0.f);       // d / d (weighted sum), fine
        const float gs0 = gb0 + (g_sharp0 ? g_sharp0[n * 3 + c] * tm_slope(s0, gamma) : 0.f);  // ... coarse
        d_rgb[t * 3 + c] = gs * w;
        d_rgb0[t * 3 + c] = gs0 * w;
        dw += gs * rgb[t * 3 + c] + gs0 * rgb0[t * 3 + c];
        if (slot == 0) d_nraw[n * 4 + c] = (gb + gb0 + (g_noise ? g_noise[n * 3 + c] : 0.f)) * 0.1f * sg * (1.f - sg);
    }
    if (slot == 0) d_nraw[n * 4 + 3] = 0.f;
    d_ccw[t] = dw;
}

// work == NULL: loss[0] is added to (the caller zeroed it).  work != NULL ({running sum, finished workgroups}, both zero on
// entry and left zero): loss[0] is WRITTEN by the last workgroup to finish -- no zero-fill launch in front (ABI 7).
__global__ void loss_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ tg,
                            int n3, float scale, float* __restrict__ loss, float* __restrict__ ga, float* __restrict__ gb,
                            float* __restrict__ work) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    float l = 0.f;
    if (t < n3) {
        const float inv = scale / (float)n3;
        const float da = a[t] - tg[t], db = b[t] - tg[t];
        l = 0.5f * (da * da + fabsf(da) + db * db + fabsf(db)) * inv;
        const float va = (da + 0.5f * (da > 0.f ? 1.f : (da < 0.f ? -1.f : 0.f))) * inv;
        const float vb = (db + 0.5f * (db > 0.f ? 1.f : (db < 0.f ? -1.f : 0.f))) * inv;
        if (gb != nullptr) { ga[t] = va; gb[t] = vb; }
        else ga[t] = va + vb;           // a and b are the same tensor (no fine pass: rgb0 = rgb): its gradient is the sum
    }
    l = wave_sum(l);
    if (work == nullptr) {
        if ((threadIdx.x & 63) == 0 && l != 0.f) atomicAdd(loss, l);
        return;
    }
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(work, part[0] + part[1] + part[2] + part[3]);
        __threadfence();
        if (atomicAdd(reinterpret_cast<unsigned*>(work) + 1, 1u) == gridDim.x - 1) {
            loss[0] = atomicExch(work, 0.f);
            reinterpret_cast<unsigned*>(work)[1] = 0u;
        }
    }
}

// ------------------------------------------------- consistency loss
// compute_mean_with_confidence (helpers:665-688) + the masked L1 of run_lushnerf.py:644-650, forward and
// backward (the mean is built with differentiable in-place adds, so gradients flow through it):
//   m[v][p] = cert[v][p] >= thr ; mean[p][c] = sum_v m rgb / max(1, sum_v m)
//   loss = sum_{v,p,c} |rgb - mean| m / #{m}
// One workgroup; thread t owns (p, c) = (t / 3, t % 3).
__global__ __launch_bounds__(256) void consist_loss_kernel(const float* __restrict__ rgb, const float* __restrict__ cert,
                                                          int V, int ns, float thr, float* __restrict__ loss,
                                                          float* __restrict__ grad) {
    __shared__ float s_cnt, s_sum;
    if (threadIdx.x == 0) { s_cnt = 0.f; s_sum = 0.f; }
    __syncthreads();
    float cnt = 0.f;
    for (int i = threadIdx.x; i < V * ns; i += blockDim.x) cnt += cert[i] >= thr ? 1.f : 0.f;
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt != 0.f) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    const float n_mask = s_cnt;                      // 0 -> loss = 0/0 = NaN, as in the reference
    float part = 0.f;
    for (int t = threadIdx.x; t < ns * 3; t += blockDim.x) {
        const int p = t / 3, c = t % 3;
        float sum = 0.f, k = 0.f;
        for (int v = 0; v < V; ++v)
            if (cert[v * ns + p] >= thr) { sum += rgb[(v * ns + p) * 3 + c]; k += 1.f; }
        const float mean = k > 0.f ? sum / k : 0.f;
        float ssum = 0.f;
        for (int v = 0; v < V; ++v)
            if (cert[v * ns + p] >= thr) {
                const float d = rgb[(v * ns + p) * 3 + c] - mean;
                part += fabsf(d);
                ssum += d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            }
        for (int v = 0; v < V; ++v) {
            float g = 0.f;
            if (cert[v * ns + p] >= thr) {
                const float d = rgb[(v * ns + p) * 3 + c] - mean;
                g = ((d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) - ssum / k) / n_mask;
            }
            grad[(v * ns + p) * 3 + c] = g;
        }
    }
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0 && part != 0.f) atomicAdd(&s_sum, part);
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = s_sum / n_mask;
}

}  // namespace lush

using namespace lush;

extern "C" {

int lush_blur_mix_fwd(const float* rgb, const float* rgb0, const float* ccw, const float* nraw, int nraw_ld, int N, int M1, int gamma,
                      float* blur, float* blur0, float* noise, float* sharp, float* sharp0, lush_stream_t st) {
    if (N < 1 || M1 < 1 || nraw_ld < 3) return set_error("lush_blur_mix_fwd: empty, or a row stride below 3");
    if (!rgb || !rgb0 || !ccw || !nraw || !blur || !blur0 || !noise || !sharp || !sharp0) return set_error("lush_blur_mix_fwd: every pointer is required");
    return launch(blur_mix_fwd_kernel, dim3(cdiv(3LL * N, 256)), dim3(256), 0, st, rgb, rgb0, ccw, nraw, nraw_ld, N, M1, gamma, blur, blur0,
                  noise, sharp, sharp0);
}
int lush_blur_mix_bwd(const float* rgb, const float* rgb0, const float* ccw, const float* nraw, int nraw_ld, int N, int M1, int gamma,
                      const float* g_blur, const float* g_blur0, const float* g_noise, const float* g_sharp, const float* g_sharp0,
                      float* d_rgb, float* d_rgb0, float* d_ccw, float* d_nraw, lush_stream_t st) {
    if (N < 1 || M1 < 1 || nraw_ld < 3) return set_error("lush_blur_mix_bwd: empty, or a row stride below 3");
    if (!rgb || !rgb0 || !ccw || !nraw || !d_rgb || !d_rgb0 || !d_ccw || !d_nraw) return set_error("lush_blur_mix_bwd: inputs and the four gradient outputs are required");
    return launch(blur_mix_bwd_kernel, dim3(cdiv((long long)N * M1, 256)), dim3(256), 0, st, rgb, rgb0, ccw, nraw, nraw_ld, N, M1, gamma,
                  g_blur, g_blur0, g_noise, g_sharp, g_sharp0, d_rgb, d_rgb0, d_ccw, d_nraw);
}

int lush_wsum_fwd(const float* x, const float* ccw, int N, int M, int C, float* y, lush_stream_t st) {
    return launch(wsum_fwd_kernel, dim3(cdiv((long long)N * C, 256)), dim3(256), 0, st, x, ccw, N, M, C, y);
}
int lush_wsum_bwd(const float* x, const float* ccw, int N, int M, int C, const float* dy, float* dx, float* dccw,
                  lush_stream_t st) {
    return launch(wsum_bwd_kernel, dim3(cdiv((long long)N * M, 256)), dim3(256), 0, st, x, ccw, N, M, C, dy, dx, dccw);
}
int lush_tonemap_fwd(const float* x, const float* nraw, int n, int gamma, float* y, lush_stream_t st) {
    return launch(tonemap_fwd_kernel, dim3(cdiv(3LL * n, 256)), dim3(256), 0, st, x, nraw, 3 * n, gamma, y);
}
int lush_tonemap_bwd(const float* x, const float* nraw, int n, int gamma, const float* dy, float* dx, float* dnraw,
                     lush_stream_t st) {
    return launch(tonemap_bwd_kernel, dim3(cdiv(3LL * n, 256)), dim3(256), 0, st, x, nraw, 3 * n, gamma, dy, dx, dnraw);
}
int lush_noise_act_fwd(const float* x, int n, float* y, lush_stream_t st) {
    return launch(noise_act_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, n, y);
}
int lush_noise_act_bwd(const float* x, int n, const float* dy, float* dx, lush_stream_t st) {
    return launch(noise_act_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, x, n, dy, dx);
}
int lush_loss_fwd_bwd(const float* a, const float* b, const float* target, int n, float scale, float* loss, float* ga,
                      float* gb, float* work, lush_stream_t st) {
    if (!gb && a != b) return set_error("lush_loss_fwd_bwd: one gradient buffer serves only a == b");
    return launch(loss_kernel, dim3(cdiv(3LL * n, 256)), dim3(256), 0, st, a, b, target, 3 * n, scale, loss, ga, gb, work);
}

int lush_consist_loss_fwd_bwd(const float* rgb, const float* cert, int V, int ns, float threshold, float* loss,
                              float* grad, lush_stream_t st) {
    if (V <= 0 || ns <= 0) return set_error("lush_consist_loss_fwd_bwd: empty");
    return launch(consist_loss_kernel, dim3(1), dim3(256), 0, st, rgb, cert, V, ns, threshold, loss, grad);
}

}  // extern "C"
