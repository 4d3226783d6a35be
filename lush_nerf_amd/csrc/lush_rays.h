// lush-march: one ray -> its row of the march's batch, and the reverse (the head of render_train_scene, models/lushnerf.py:772-795).
// Shared by lush_rays.hip (rays the caller holds) and lush_rbk.hip (rays warped in registers): the same bits either way.
#pragma once
#include "lush_common.h"

namespace lush {

// one ray (o, d) -> its 11 batch columns [o' d' near far viewdir]
__device__ __forceinline__ void pack_one(const float (&o)[3], const float (&d)[3], int ndc, float cx, float cy, float near, float far,
                                         float* __restrict__ b) {
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    b[8] = d[0] / nrm; b[9] = d[1] / nrm; b[10] = d[2] / nrm;
    if (ndc) {   // utils/run_lushnerf_helpers.py:542-562 with near = 1
        const float t = -(1.f + o[2]) / d[2];
        const float px = __fadd_rn(o[0], __fmul_rn(t, d[0])), py = __fadd_rn(o[1], __fmul_rn(t, d[1])),
                    pz = __fadd_rn(o[2], __fmul_rn(t, d[2]));
        b[0] = __fmul_rn(cx, px) / pz;
        b[1] = __fmul_rn(cy, py) / pz;
        b[2] = 1.f + 2.f / pz;
        b[3] = __fmul_rn(cx, __fsub_rn(d[0] / d[2], px / pz));
        b[4] = __fmul_rn(cy, __fsub_rn(d[1] / d[2], py / pz));
        b[5] = -2.f / pz;
    } else {
        b[0] = o[0]; b[1] = o[1]; b[2] = o[2]; b[3] = d[0]; b[4] = d[1]; b[5] = d[2];
    }
    b[6] = near; b[7] = far;
}
// reverse mode of pack_one: g = d loss / d (batch row) -> go, gd (overwritten)
__device__ __forceinline__ void pack_one_bwd(const float (&o)[3], const float (&d)[3], int ndc, float cx, float cy,
                                             const float* __restrict__ g, float (&go)[3], float (&gd)[3]) {
    go[0] = go[1] = go[2] = 0.f;
    gd[0] = gd[1] = gd[2] = 0.f;
    // viewdir = d/|d|
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float v[3] = {d[0] / nrm, d[1] / nrm, d[2] / nrm};
    const float vg = v[0] * g[8] + v[1] * g[9] + v[2] * g[10];
#pragma unroll
    for (int i = 0; i < 3; ++i) gd[i] += (g[8 + i] - v[i] * vg) / nrm;
    if (ndc) {
        const float t = -(1.f + o[2]) / d[2];
        const float px = o[0] + t * d[0], py = o[1] + t * d[1], pz = o[2] + t * d[2];
        const float ipz = 1.f / pz, ipz2 = ipz * ipz, idz = 1.f / d[2];
        const float gpx = cx * ipz * (g[0] - g[3]);
        const float gpy = cy * ipz * (g[1] - g[4]);
        const float gpz = ipz2 * (-cx * px * (g[0] - g[3]) - cy * py * (g[1] - g[4]) - 2.f * g[2] + 2.f * g[5]);
        gd[0] += cx * g[3] * idz;
        gd[1] += cy * g[4] * idz;
        gd[2] += -(cx * d[0] * g[3] + cy * d[1] * g[4]) * idz * idz;
        const float gp[3] = {gpx, gpy, gpz};
        float gt = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) { go[i] += gp[i]; gd[i] += t * gp[i]; gt += gp[i] * d[i]; }
        go[2] += -gt * idz;
        gd[2] += -gt * t * idz;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) { go[i] += g[i]; gd[i] += g[3 + i]; }
    }
}

}  // namespace lush
