// fbsmi_kf_em.hip -- the front of fbsmi_kf_sample / fbsmi_kfs_sample for a model whose forward process is Euler-Maruyama
// (include/fbsmi.h, fbsmi_kf_set_em_forward; the Gaussian Schrodinger bridge, experiments/sb/filter.py:137-148): the
// observation path is the y half of a joint (x, y) path from a drawn x0 -- the front of fbsmi_lg_fsamp_create_em
// (fbsmi_lg.hip, k_fs_front_em) on the same keys, writing into the Kalman handle's vs and m_0.
//
// A translation unit of its own: the kernels of fbsmi_kf.hip keep the code they had (the optimiser's choices inside the
// Threefry schedule of the drawing kernels there move with what else the module holds).
#include "fbsmi_device.h"
#include "fbsmi_em_path.h"
#include "fbsmi_kf_em.h"

namespace fbsmi {

namespace {

// keys, x0, the joint path by em_path_run from concat(x0, y0) with its y half written reversed into vs, and the conditional
// mean of k_kf_front's tail (the same expression and order).  One workgroup per sample, thread i < D = du + dv owns
// coordinate i; the block is D rounded up to a wave.  The T interval keys split(key_em, T) are derived once, a thread per
// interval, into LDS (SLAB: into the handle's ekeys); the noise of sub-step (k, j) is drawn by the thread that consumes it,
// where em_path_run asks for it -- one sub-step ahead of its use -- and no noise buffer exists.  Nothing global sits on the
// T * nsub dependent chain; the x half of the path is never stored.
// LDS: 8 KB of keys, 2 KB of xs, 2 KB of z and yT (12 304 bytes; SLAB 4 112); the M row of a thread is 2 * kEmChunk
// registers.
template <bool SLAB>
__global__ void __launch_bounds__(kEmPathMaxD) k_kf_front_em(KfEmFront d, const uint32_t* __restrict__ keys,
                                                             const float* __restrict__ y0) {
    __shared__ float xs[2 * kEmPathMaxD];
    __shared__ uint32_t sk[4];
    __shared__ uint32_t skeys[SLAB ? 2 : 2 * kKfEmKeysLds];
    __shared__ float sz[kEmPathMaxD], syT[kEmPathMaxD];
    const int b = blockIdx.x, i = threadIdx.x;
    const int T = d.T, du = d.du, dv = d.dv, D = du + dv;
    if (i == 0) {
        uint32_t f0, f1;
        split_at(keys[2 * b], keys[2 * b + 1], 3, 0, f0, f1);            // key_fwd
        split_at(f0, f1, 2, 0, sk[0], sk[1]);                            // key_x0
        split_at(f0, f1, 2, 1, sk[2], sk[3]);                            // key_em
    }
    __syncthreads();
    uint32_t* kk = SLAB ? d.ekeys + (size_t)b * T * 2 : skeys;
    for (int k = i; k < T; k += blockDim.x) split_at(sk[2], sk[3], T, k, kk[2 * k], kk[2 * k + 1]);
    const bool proper = d.x0_chol != nullptr;
    float x = 0.0f;
    if (i < du) {
        x = normal_at(sk[0], sk[1], (uint64_t)du, (uint64_t)i);          // normal(key_x0, (du,))
        sz[i] = x;
    } else if (i < D) {
        x = y0[i - du];
    }
    __syncthreads();                                                     // the interval keys and z are in place
    if (proper && i < du) {
        float acc = sz[0] * d.x0_chol[i];
        for (int c = 1; c < du; ++c) acc = acc + sz[c] * d.x0_chol[(size_t)c * du + i];
        x = d.x0_mean[i] + acc;
    }
    float* vs = d.vs + (size_t)b * ((size_t)T + 1) * dv;
    const int col = i - du;
    if (i >= du && i < D) vs[(size_t)T * dv + col] = x;                  // vs[T] = y0
    const EmTables t{d.nsub, d.M, d.c, d.ddt, d.s};
    const uint64_t n = (uint64_t)d.nsub * (uint64_t)D;
    float last = x;
    em_path_run(t, T, D, x, xs,
                [&](int k, int j) { return normal_at(kk[2 * k], kk[2 * k + 1], n, (uint64_t)j * D + i); },
                [&](int k, float v) {                                    // (em_path_run calls emit for i < D only)
                    if (i >= du) vs[(size_t)(T - 1 - k) * dv + col] = v;
                    last = v;
                });
    if (i >= du && i < D) syT[col] = last;                               // yT = vs[0]
    __syncthreads();
    for (int u = i; u < du; u += blockDim.x) {
        double s = 0.0;
        for (int cc = 0; cc < dv; ++cc) s = s + d.gain[(size_t)u * dv + cc] * ((double)syT[cc] - d.m_v[cc]);
        d.m0[(size_t)b * du + u] = (float)(d.m_u[u] + s);
    }
}

}  // namespace

void kf_front_em_launch(const KfEmFront& f, const uint32_t* keys, const float* y0, int B, hipStream_t st) {
    const int block = (f.du + f.dv + 63) / 64 * 64;
    if (f.ekeys) k_kf_front_em<true><<<B, block, 0, st>>>(f, keys, y0);
    else k_kf_front_em<false><<<B, block, 0, st>>>(f, keys, y0);
}

}  // namespace fbsmi
