// fbsmi_em_path.h -- the matrix-affine Euler-Maruyama path of include/fbsmi.h (fbsmi_em_forward), shared by the
// stand-alone kernel (fbsmi_sde.hip, fbsmi_lg_em_path) and the in-sweep forward process of the fused Gibbs sweep
// (fbsmi_lg.hip, fbsmi_lg_sweep_set_em_forward).
//
// One workgroup runs one path; thread i < D owns coordinate i.  The recurrence is T*nsub dependent sub-steps, each a D x D
// matvec; x crosses threads through LDS (double-buffered: one barrier per sub-step; a single wave when D <= 64).  Nothing
// global sits on the dependent chain: the M row of thread i is streamed in chunks of kEmChunk registers one chunk ahead
// (for D <= kEmChunk the whole row of the NEXT sub-step is in flight while the current one is folded in), and c, s, the
// noise and ddt of the next sub-step are fetched while the current one runs.
#pragma once

#include "fbsmi_device.h"

namespace fbsmi {

constexpr int kEmPathMaxD = 256;   // du, dv <= 128 in the fused sweep
constexpr int kEmChunk = 32;

struct EmTables {
    int nsub;
    const float* M;    // [T*nsub][D][D]
    const float* c;    // [T*nsub][D]
    const float* ddt;  // [T]
    const float* s;    // [T*nsub]
};

// noise(k, j) -> xi_k[j][i] of this thread's coordinate; emit(k, x) receives x_i after interval k (threads i < D only).
// blockDim.x must be a multiple of 64 and at least D; xs is LDS of 2 * kEmPathMaxD floats.
template <typename Noise, typename Emit>
__device__ __forceinline__ void em_path_run(const EmTables& t, int T, int D, float x, float* xs, Noise&& noise, Emit&& emit) {
    const int i = threadIdx.x;
    const bool on = i < D;
    const int nsub = t.nsub;
    const int R = T * nsub;
    const int nch = (D + kEmChunk - 1) / kEmChunk;
    const size_t DD = (size_t)D * D;
    const float* Mi = t.M + (size_t)(on ? i : 0) * D;
    float cur[kEmChunk], nxt[kEmChunk] = {};
    auto load = [&](int r, int cb, float (&buf)[kEmChunk]) {
        const float* src = Mi + (size_t)r * DD + (size_t)cb * kEmChunk;
#pragma unroll
        for (int q = 0; q < kEmChunk; ++q) buf[q] = (on && cb * kEmChunk + q < D) ? src[q] : 0.0f;
    };
    if (on) xs[i] = x;
    load(0, 0, cur);
    float c_n = on ? t.c[i] : 0.0f, s_n = t.s[0], z_n = on ? noise(0, 0) : 0.0f;
    float h = t.ddt[0], h_n = h;
    __syncthreads();
    int p = 0, k = 0, j = 0;
    for (int r = 0; r < R; ++r) {
        const float cr = c_n, sr = s_n, zr = z_n;
        int j1 = j + 1, k1 = k;
        if (j1 == nsub) { j1 = 0; ++k1; }
        if (r + 1 < R) {   // operands of sub-step r + 1: off the chain
            c_n = on ? t.c[(size_t)(r + 1) * D + i] : 0.0f;
            s_n = t.s[r + 1];
            z_n = on ? noise(k1, j1) : 0.0f;
            if (j1 == 0) h_n = t.ddt[k1];
        }
        const float* xp = xs + p * kEmPathMaxD;
        float acc = cr;   // f_i = c_i + sum_c M_ic x_c, one fmaf chain in c order
        for (int cb = 0; cb < nch; ++cb) {
            if (cb + 1 < nch) load(r, cb + 1, nxt);
            else if (r + 1 < R) load(r + 1, 0, nxt);
#pragma unroll
            for (int q = 0; q < kEmChunk; ++q)
                if (cb * kEmChunk + q < D) acc = fbsmi_fmaf(cur[q], xp[cb * kEmChunk + q], acc);
#pragma unroll
            for (int q = 0; q < kEmChunk; ++q) cur[q] = nxt[q];
        }
        if (on) {
            x = (x + acc * h) + sr * zr;
            xs[(p ^ 1) * kEmPathMaxD + i] = x;
        }
        __syncthreads();
        p ^= 1;
        if (j1 == 0) {
            if (on) emit(k, x);
            h = h_n;
        }
        j = j1;
        k = k1;
    }
}

}  // namespace fbsmi
