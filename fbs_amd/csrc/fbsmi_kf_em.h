// fbsmi_kf_em.h -- the Euler-Maruyama front of the fused Kalman sampler (fbsmi_kf_set_em_forward): what fbsmi_kf.hip hands
// to the launch in fbsmi_kf_em.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fbsmi {

constexpr int kKfEmKeysLds = 1024;    // intervals whose keys a workgroup keeps in LDS (8 KB)

// what the front launch reads and writes (the handle's pointers)
struct KfEmFront {
    int du, dv, T, nsub;
    const float *M, *c, *ddt, *s;     // fbsmi_em_forward's tables
    const float *x0_mean, *x0_chol;   // the handle's copies; (du), (du, du) lower factor: x0 = mean + z @ chol; both null: x0 = z
    uint32_t* ekeys;                  // [B][T][2] interval keys of a handle with T > kKfEmKeysLds, else null
    const double *m_u, *m_v, *gain;   // (du) (dv) (du, dv)
    float* vs;                        // [B][T+1][dv]
    float* m0;                        // [B][du]
};

// one workgroup per sample of the batch on `st`: keys [B][2], y0 (dv); du + dv <= 256
void kf_front_em_launch(const KfEmFront& f, const uint32_t* keys, const float* y0, int B, hipStream_t st);

}  // namespace fbsmi
