// lush-march: what a training step needs besides rays and networks + its C ABI -- the march's random draws (torch.rand /
// randn_like of models/lushnerf.py:515, :322 and helpers:578, as one Philox launch), torch.optim.Adam's step, and the
// device-side step state that lets a captured step advance.
#include "lush_common.h"
#include "lush_host.h"
#include "../../include/lush_march.h"

#include <cmath>

namespace lush {

// ------------------------------------------------------------------ random draws
// The four draws of one march (models/lushnerf.py:515 torch.rand [R,Ns]; :322 torch.randn_like [R,Ns-1]; helpers:578
// torch.rand [R,Ni]; :322 [R,Ns+Ni-1]) in ONE launch: Philox4x32-10 counter RNG, key = (seed, stream), counter = (element
// quad, array id, call offset).  Uniforms are 24-bit in [0, 1) as torch.rand's; normals are Box-Muller pairs.  The
// reference's own torch RNG stream cannot be reproduced (it differs between CPU and GPU builds of torch itself);
// parity tests pass explicit draws instead.
__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
struct DrawArr { float* p; long long n; int normal; };
struct DrawSet { DrawArr a[4]; };
__global__ void draws_kernel(DrawSet S, unsigned long long seed, unsigned long long offset, long long total_quads,
                             const unsigned long long* __restrict__ base_dev) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total_quads) return;
    if (base_dev) offset += *base_dev;          // the step state's draw counter (lush_step_state): a captured launch still advances
    long long base = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long nq = (S.a[i].n + 3) / 4;
        if (q >= base && q < base + nq) {
            const long long e = q - base;
            unsigned c[4] = {(unsigned)e, (unsigned)(e >> 32), (unsigned)i, (unsigned)offset};
            philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32) ^ (unsigned)(offset >> 32));
            float v[4];
            if (S.a[i].normal) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float u1 = ((float)(c[2 * h] >> 8) + 1.0f) * 5.9604644775390625e-08f;          // (0, 1]
                    const float u2 = (float)(c[2 * h + 1] >> 8) * 5.9604644775390625e-08f;                // [0, 1)
                    const float rad = sqrtf(-2.0f * logf(u1));
                    float sn, cs;
                    sincosf(6.283185307179586f * u2, &sn, &cs);
                    v[2 * h] = rad * cs;
                    v[2 * h + 1] = rad * sn;
                }
            } else {
#pragma unroll
                for (int h = 0; h < 4; ++h) v[h] = (float)(c[h] >> 8) * 5.9604644775390625e-08f;          // [0, 1), 24 bits
            }
#pragma unroll
            for (int h = 0; h < 4; ++h)
                if (4 * e + h < S.a[i].n) S.a[i].p[4 * e + h] = v[h];
        }
        base += nq;
    }
}

// ------------------------------------------------------------------------ Adam
// element i of torch.optim.Adam's step (bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t))
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, long long i, float lr, float b1, float b2, float eps,
                                            float bc1, float bc2_sqrt, float gscale) {
    const float gi = g[i] * gscale;
    const float mi = m[i] + (gi - m[i]) * (1.f - b1);          // torch: exp_avg.lerp_(grad, 1-beta1)
    const float vi = v[i] * b2 + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] -= (lr / bc1) * (mi / denom);
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float lr, float b1, float b2, float eps, float bc1,
                            float bc2_sqrt, float gscale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) adam_update(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2_sqrt, gscale);
}

// Step state on the device (include/lush_march.h lush_step_state): what a training step takes from the host as kernel
// arguments otherwise -- learning rate, Adam's step counts (as their bias corrections), the Philox draw counter -- so that
// a step captured in a HIP graph advances when it is replayed.
struct StepState {
    unsigned long long draw_base;   // draw calls made before this step
    int global_step;                // steps taken
    int steps[3];                   // Adam steps taken per segment
    float lr;                       // rate of the next step: lrate * 0.1 ** (max(global_step - 1, 0) / decay_steps)
    float bc1[3], bc2s[3];          // 1 - beta1^t, sqrt(1 - beta2^t) of the next step (t = steps + 1) per segment
};
__global__ void adam_state_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, long long n, const StepState* __restrict__ st, int seg, float b1,
                                  float b2, float eps, float gscale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) adam_update(p, g, m, v, i, st->lr, b1, b2, eps, st->bc1[seg], st->bc2s[seg], gscale);
}
// the same update over SEVERAL segments of one flat buffer in one launch: element i belongs to segment (i >= end0) + (i >= end1);
// segments whose bit is clear in `mask` are left alone (the reference's grad=None parameters: Adam skips them, counts included)
__global__ void adam_state_multi_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                        float* __restrict__ v, long long end0, long long end1, long long end2,
                                        const StepState* __restrict__ st, int mask, float b1, float b2, float eps, float gscale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end2) return;
    const int seg = (i >= end0) + (i >= end1);
    if (!((mask >> seg) & 1)) return;
    adam_update(p, g, m, v, i, st->lr, b1, b2, eps, st->bc1[seg], st->bc2s[seg], gscale);
}
struct AdamMulti { long long end[3]; float bc1[3], bc2s[3]; int mask; };
__global__ void adam_multi_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                  const AdamMulti A, float lr, float b1, float b2, float eps, float gscale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.end[2]) return;
    const int seg = (i >= A.end[0]) + (i >= A.end[1]);
    if (!((A.mask >> seg) & 1)) return;
    const float bc1 = seg == 0 ? A.bc1[0] : seg == 1 ? A.bc1[1] : A.bc1[2];
    const float bc2_sqrt = seg == 0 ? A.bc2s[0] : seg == 1 ? A.bc2s[1] : A.bc2s[2];
    adam_update(p, g, m, v, i, lr, b1, b2, eps, bc1, bc2_sqrt, gscale);
}
__device__ void step_state_derive(StepState* st, double lrate, double decay_steps, double b1, double b2) {
    const int g = st->global_step - 1 > 0 ? st->global_step - 1 : 0;
    st->lr = (float)(lrate * pow(0.1, (double)g / decay_steps));
    for (int s = 0; s < 3; ++s) {
        const double t = (double)(st->steps[s] + 1);
        st->bc1[s] = (float)(1.0 - pow(b1, t));
        st->bc2s[s] = (float)sqrt(1.0 - pow(b2, t));
    }
}
__global__ void step_state_advance_kernel(StepState* st, int n_draw_calls, int active_mask, double lrate, double decay_steps,
                                          double b1, double b2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->draw_base += (unsigned long long)n_draw_calls;
    for (int s = 0; s < 3; ++s)
        if ((active_mask >> s) & 1) st->steps[s] += 1;
    st->global_step += 1;
    step_state_derive(st, lrate, decay_steps, b1, b2);
}
__global__ void step_state_init_kernel(StepState* st, unsigned long long draw_base, int global_step, int s0, int s1, int s2,
                                       double lrate, double decay_steps, double b1, double b2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->draw_base = draw_base; st->global_step = global_step;
    st->steps[0] = s0; st->steps[1] = s1; st->steps[2] = s2;
    step_state_derive(st, lrate, decay_steps, b1, b2);
}

}  // namespace lush

using namespace lush;

// the multi-segment launches run only up to the end of the last active segment
static long long adam_active_end(int mask, long long end0, long long end1, long long end2) {
    return (mask & 4) ? end2 : (mask & 2) ? end1 : (mask & 1) ? end0 : 0;
}

extern "C" {

static int draws_impl(unsigned long long seed, unsigned long long offset, const unsigned long long* base_dev, float* t_rand,
                      long long n_t, float* noise_c, long long n_c, float* u, long long n_u, float* noise_f, long long n_f,
                      lush_stream_t st) {
    DrawSet S{};
    S.a[0] = {t_rand, t_rand ? n_t : 0, 0};
    S.a[1] = {noise_c, noise_c ? n_c : 0, 1};
    S.a[2] = {u, u ? n_u : 0, 0};
    S.a[3] = {noise_f, noise_f ? n_f : 0, 1};
    long long quads = 0;
    for (int i = 0; i < 4; ++i) quads += (S.a[i].n + 3) / 4;
    if (quads == 0) return 0;
    return launch(draws_kernel, dim3(cdiv(quads, 256)), dim3(256), 0, st, S, seed, offset, quads, base_dev);
}
int lush_draws(unsigned long long seed, unsigned long long offset, float* t_rand, long long n_t, float* noise_c,
               long long n_c, float* u, long long n_u, float* noise_f, long long n_f, lush_stream_t st) {
    return draws_impl(seed, offset, nullptr, t_rand, n_t, noise_c, n_c, u, n_u, noise_f, n_f, st);
}
int lush_draws_state(unsigned long long seed, unsigned long long offset, const void* state, float* t_rand, long long n_t,
                     float* noise_c, long long n_c, float* u, long long n_u, float* noise_f, long long n_f, lush_stream_t st) {
    if (!state) return set_error("lush_draws_state: the step state is required");
    return draws_impl(seed, offset, &static_cast<const StepState*>(state)->draw_base, t_rand, n_t, noise_c, n_c, u, n_u, noise_f, n_f, st);
}

int lush_adam(float* param, const float* grad, float* m, float* v, long long n, float lr, float beta1, float beta2,
              float eps, int step, float grad_scale, lush_stream_t st) {
    if (n <= 0) return 0;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    return launch(adam_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, param, grad, m, v, n, lr, beta1, beta2, eps, bc1, bc2s, grad_scale);
}

int lush_adam_multi(float* param, const float* grad, float* m, float* v, long long end0, long long end1, long long end2, int mask,
                    float lr, float beta1, float beta2, float eps, const int* steps, float grad_scale, lush_stream_t st) {
    if (!steps || end0 < 0 || end1 < end0 || end2 < end1 || mask < 0 || mask > 7) return set_error("lush_adam_multi: bad segment ends / mask / steps");
    AdamMulti A;
    A.end[0] = end0; A.end[1] = end1;
    A.end[2] = adam_active_end(mask, end0, end1, end2);
    A.mask = mask;
    for (int s = 0; s < 3; ++s) {
        const int t = steps[s] > 0 ? steps[s] : 1;
        A.bc1[s] = (float)(1.0 - pow((double)beta1, (double)t));
        A.bc2s[s] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    }
    if (A.end[2] <= 0) return 0;
    return launch(adam_multi_kernel, dim3(cdiv(A.end[2], 256)), dim3(256), 0, st, param, grad, m, v, A, lr, beta1, beta2, eps, grad_scale);
}

size_t lush_step_state_bytes(void) { return sizeof(StepState); }
int lush_step_state_init(void* state, unsigned long long draw_base, int global_step, const int* adam_steps, double lrate,
                         double decay_steps, double beta1, double beta2, lush_stream_t st) {
    if (!state || !adam_steps) return set_error("lush_step_state_init: null argument");
    return launch(step_state_init_kernel, dim3(1), dim3(1), 0, st, static_cast<StepState*>(state), draw_base, global_step,
                  adam_steps[0], adam_steps[1], adam_steps[2], lrate, decay_steps, beta1, beta2);
}
int lush_step_state_advance(void* state, int n_draw_calls, int active_mask, double lrate, double decay_steps, double beta1,
                            double beta2, lush_stream_t st) {
    if (!state) return set_error("lush_step_state_advance: null state");
    return launch(step_state_advance_kernel, dim3(1), dim3(1), 0, st, static_cast<StepState*>(state), n_draw_calls,
                  active_mask, lrate, decay_steps, beta1, beta2);
}
int lush_adam_state(float* param, const float* grad, float* m, float* v, long long n, const void* state, int segment,
                    float beta1, float beta2, float eps, float grad_scale, lush_stream_t st) {
    if (n <= 0) return 0;
    if (!state || segment < 0 || segment > 2) return set_error("lush_adam_state: bad state / segment");
    return launch(adam_state_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, param, grad, m, v, n,
                  static_cast<const StepState*>(state), segment, beta1, beta2, eps, grad_scale);
}

int lush_adam_state_multi(float* param, const float* grad, float* m, float* v, long long end0, long long end1, long long end2,
                          const void* state, int mask, float beta1, float beta2, float eps, float grad_scale, lush_stream_t st) {
    if (!state || end0 < 0 || end1 < end0 || end2 < end1 || mask < 0 || mask > 7) return set_error("lush_adam_state_multi: bad state / segment ends / mask");
    const long long n = adam_active_end(mask, end0, end1, end2);
    if (n <= 0) return 0;
    return launch(adam_state_multi_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, param, grad, m, v, end0, end1, n,
                  static_cast<const StepState*>(state), mask, beta1, beta2, eps, grad_scale);
}

}  // extern "C"
