// fbsmi_train.hip -- the per-step work round the score network of the denoising score-matching trainer
// (fbs/sdes/linear.py:230-360 make_linear_sde_law_loss, fbs/nn/utils.py:60-83 make_optax_kernel; fbs_amd/sdes/losses.py,
// fbs_amd/train.py).  The arithmetic of every entry is specified in include/fbsmi.h.
//
//   fbsmi_uniform_host         fbsmi_uniform on the host (the trainer's random times)
//   fbsmi_dsm_noise_batched    xt[b] = F[b] data[idx[b]] + sq[b] normal(keys[b], (D,)): gather, draw and noising in one pass
//   fbsmi_dsm_loss_batched     the loss, its row sums and d loss / d net in one pass over the network output
//   fbsmi_sqnorm               sum of squares of a flat vector (the global gradient norm of the clip), canonical tree
//   fbsmi_adam_ema_step        optax's clip_by_global_norm + adam + the reference's ema_kernel in one pass
//
// Reductions.  A row (or the flat vector) is cut into aligned chunks of kChunk = 2048 elements, eight consecutive
// elements per thread of a 256-thread workgroup: chunk_total<8>, then block_upsweep, give the root of the canonical
// pairwise tree of the chunk (zero beyond the end: x + 0 is exact).  A row's chunks are spread over up to 64 workgroups,
// which loop when there are more chunks than that.  One small launch finishes: a thread folds the chunk roots of a row
// with a binary-counter stack, which performs exactly the additions of the pairwise tree over the zero-padded index, then
// the rows of an aligned power-of-two block likewise, and block_upsweep joins the 256 blocks.  The result is the tree of
// fbsmi_sum whatever the tiling was.
//
// The loss kernel in mode 0 redraws element e of normal(keys[b], (D,)) with one block-cipher call per element (the
// partner word belongs to element e +- D/2, which lies in another chunk); the noise kernel, which has no tree to respect,
// uses both words of each call.  gfx950 only.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"

namespace fbsmi {

namespace {

#define FBSMI_NEED(cond, msg) \
    if (!(cond)) return fail(FBSMI_ERR_ARG, msg)

#define FBSMI_LAUNCH_CHECK()                                                     \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) return fail(FBSMI_ERR_HIP, hipGetErrorString(e_)); \
    } while (0)

constexpr int kItems = 8;                       // consecutive elements per thread: 16 bytes of bfloat16, 2 x 16 of float32
constexpr int kChunk = kBlock * kItems;         // elements per workgroup and round
constexpr int kMaxRowGroups = 64;               // workgroups one row spreads over
constexpr int kMaxFlatGroups = 4096;            // workgroups of the flat kernels (they loop beyond)
constexpr int kLevels = 24;                     // binary-counter levels of the finishing fold: 2^24 leaves per thread
constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;
constexpr int64_t kMaxDraw = ((int64_t)1 << 32) - 4;

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) { return fbsmi_u2f((uint32_t)h << 16); }

// round to nearest even; NaN stays NaN
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
    const uint32_t u = fbsmi_f2u(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return (uint32_t)f32_to_bf16_bits(lo) | ((uint32_t)f32_to_bf16_bits(hi) << 16);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ------------------------------------------------------------------------------------------------
// noising: a thread owns elements i and i + half of a row (the two words of one cipher call), four consecutive i when
// the row allows 16-byte accesses (D a multiple of 8: then half is a multiple of 4 and D is even)
// ------------------------------------------------------------------------------------------------
template <int OUTDT>
__device__ __forceinline__ void store_xt(void* xt, int64_t at, float v) {
    if (OUTDT == 0) ((float*)xt)[at] = v;
    else ((unsigned short*)xt)[at] = f32_to_bf16_bits(v);
}

template <int OUTDT>
__device__ __forceinline__ void store_xt4(void* xt, int64_t at, const float (&v)[4]) {
    if (OUTDT == 0) *(float4*)((float*)xt + at) = make_float4(v[0], v[1], v[2], v[3]);
    else *(uint2*)((unsigned short*)xt + at) = make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]));
}

template <int OUTDT, bool VEC>
__global__ void __launch_bounds__(kBlock) k_dsm_noise(const float* __restrict__ data, const int32_t* __restrict__ idx,
                                                      const uint32_t* __restrict__ keys, const float* __restrict__ F,
                                                      const float* __restrict__ sq, uint64_t D, int bpr,
                                                      void* __restrict__ xt) {
    const int64_t b = blockIdx.x / bpr;
    const int q = (int)(blockIdx.x - b * bpr);
    const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
    const float f = F[b], s = sq[b];
    const float* __restrict__ x0 = data + (idx ? (int64_t)idx[b] : b) * (int64_t)D;
    const int64_t row = b * (int64_t)D;
    const uint64_t half = (D + 1) >> 1;
    if (VEC) {
        for (uint64_t i = ((uint64_t)q * kBlock + threadIdx.x) * 4; i < half; i += (uint64_t)bpr * kBlock * 4) {
            const float4 a = *(const float4*)(x0 + i), c = *(const float4*)(x0 + i + half);
            const float xa[4] = {a.x, a.y, a.z, a.w}, xc[4] = {c.x, c.y, c.z, c.w};
            float oa[4], oc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                uint32_t lo, hi;
                random_bits_pair(k0, k1, D, i + u, lo, hi);
                oa[u] = f * xa[u] + s * normal_from_bits(lo);
                oc[u] = f * xc[u] + s * normal_from_bits(hi);
            }
            store_xt4<OUTDT>(xt, row + (int64_t)i, oa);
            store_xt4<OUTDT>(xt, row + (int64_t)(i + half), oc);
        }
    } else {
        for (uint64_t i = (uint64_t)q * kBlock + threadIdx.x; i < half; i += (uint64_t)bpr * kBlock) {
            const uint64_t j = i + half;
            uint32_t lo, hi;
            random_bits_pair_padded(k0, k1, D, i, lo, hi);
            store_xt<OUTDT>(xt, row + (int64_t)i, f * x0[i] + s * normal_from_bits(lo));
            if (j < D) store_xt<OUTDT>(xt, row + (int64_t)j, f * x0[j] + s * normal_from_bits(hi));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// loss
// ------------------------------------------------------------------------------------------------
struct DsmLossArgs {
    const void* net;
    const uint32_t* keys;
    const float* xt;
    const float* data;
    const int32_t* idx;
    const float* F;
    const float* sq;
    const float* gc;
    void* dnet;
    float* part;      // (B, nch) chunk roots
    uint64_t D;
    int nch, wpr;
};

// eight consecutive floats from p + at; elements at or beyond `end` read as 0
template <bool VEC>
__device__ __forceinline__ void load8_f32(const float* __restrict__ p, int64_t base, uint64_t e0, uint64_t end, float (&v)[kItems]) {
    if (VEC) {
        if (e0 < end) {   // VEC: end is a multiple of 8, so the eight are inside
            const float4 a = *(const float4*)(p + base + (int64_t)e0), c = *(const float4*)(p + base + (int64_t)e0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < kItems; ++i) v[i] = 0.0f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kItems; ++i) v[i] = e0 + i < end ? p[base + (int64_t)(e0 + i)] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void load8_bf16(const unsigned short* __restrict__ p, int64_t base, uint64_t e0, uint64_t end,
                                           float (&v)[kItems]) {
    if (VEC) {
        if (e0 < end) {
            const uint4 a = *(const uint4*)(p + base + (int64_t)e0);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = fbsmi_u2f(w[i] << 16);
                v[2 * i + 1] = fbsmi_u2f(w[i] & 0xffff0000u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kItems; ++i) v[i] = 0.0f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kItems; ++i) v[i] = e0 + i < end ? bf16_bits_to_f32(p[base + (int64_t)(e0 + i)]) : 0.0f;
    }
}

template <int NETDT, bool VEC>
__device__ __forceinline__ void store8(void* __restrict__ p, int64_t base, uint64_t e0, uint64_t end, const float (&v)[kItems]) {
    if (VEC) {
        if (e0 < end) {
            if (NETDT == 0) {
                float* o = (float*)p + base + (int64_t)e0;
                *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
                *(float4*)(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
            } else {
                *(uint4*)((unsigned short*)p + base + (int64_t)e0) =
                    make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            if (e0 + i < end) {
                if (NETDT == 0) ((float*)p)[base + (int64_t)(e0 + i)] = v[i];
                else ((unsigned short*)p)[base + (int64_t)(e0 + i)] = f32_to_bf16_bits(v[i]);
            }
        }
    }
}

template <int NETDT, int MODE, bool VEC>
__global__ void __launch_bounds__(kBlock) k_dsm_loss(DsmLossArgs a) {
    __shared__ float lds4[4];
    const int64_t b = blockIdx.x / a.wpr;
    const int q = (int)(blockIdx.x - b * a.wpr);
    const uint64_t D = a.D;
    const float sq = a.sq[b], gc = a.gc[b];
    const int64_t row = b * (int64_t)D;
    uint32_t k0 = 0, k1 = 0;
    float f = 0.0f, rsq = 0.0f;
    int64_t row0 = 0;
    if (MODE == 0) {
        k0 = a.keys[2 * b];
        k1 = a.keys[2 * b + 1];
    } else {
        f = a.F[b];
        rsq = 1.0f / sq;
        row0 = (a.idx ? (int64_t)a.idx[b] : b) * (int64_t)D;
    }
    for (int c = q; c < a.nch; c += a.wpr) {   // the same trip count for every thread of the workgroup
        const uint64_t e0 = (uint64_t)c * kChunk + (uint64_t)threadIdx.x * kItems;
        float nv[kItems], ev[kItems];
        if (NETDT == 0) load8_f32<VEC>((const float*)a.net, row, e0, D, nv);
        else load8_bf16<VEC>((const unsigned short*)a.net, row, e0, D, nv);
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < kItems; ++i) ev[i] = e0 + i < D ? normal_from_bits(random_bits_at(k0, k1, D, e0 + i)) : 0.0f;
        } else {
            float xv[kItems], dv[kItems];
            load8_f32<VEC>(a.xt, row, e0, D, xv);
            load8_f32<VEC>(a.data, row0, e0, D, dv);
#pragma unroll
            for (int i = 0; i < kItems; ++i) {
                const float num = xv[i] - f * dv[i];
                ev[i] = div_by_in_range(num) ? div_by(num, sq, rsq) : num / sq;
            }
        }
        float r2[kItems], dn[kItems];
#pragma unroll
        for (int i = 0; i < kItems; ++i) {
            const float r = sq * nv[i] + ev[i];
            r2[i] = e0 + i < D ? r * r : 0.0f;
            dn[i] = gc * r;
        }
        store8<NETDT, VEC>(a.dnet, row, e0, D, dn);
        TreePath path;
        const float tot = block_upsweep(chunk_total<kItems>(r2), path, lds4);
        if (threadIdx.x == 0) a.part[b * (int64_t)a.nch + c] = tot;
    }
}

// squares of a flat vector, chunk roots into part[0, nch)
template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_sq_chunks(const float* __restrict__ x, uint64_t n, int64_t nch,
                                                      float* __restrict__ part) {
    __shared__ float lds4[4];
    for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const uint64_t e0 = (uint64_t)c * kChunk + (uint64_t)threadIdx.x * kItems;
        float v[kItems];
        if (VEC && e0 + kItems <= n) {
            const float4 a = *(const float4*)(x + e0), b = *(const float4*)(x + e0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < kItems; ++i) v[i] = e0 + i < n ? x[e0 + i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < kItems; ++i) v[i] = v[i] * v[i];
        TreePath path;
        const float tot = block_upsweep(chunk_total<kItems>(v), path, lds4);
        if (threadIdx.x == 0) part[c] = tot;
    }
}

// The pairwise tree over the zero-padded index, fed one leaf at a time: lvl[k] holds the finished aligned block of 2^k
// leaves that waits for its right sibling (bit k of the count).  A new leaf merges upwards while blocks wait; at the end
// the waiting blocks fold from the smallest up, which is what the zero padding leaves of the tree (block + 0 = block).
struct TreeFold {
    float lvl[kLevels];
    uint32_t cnt = 0;

    __device__ __forceinline__ void push(float v) {
        bool done = false;
#pragma unroll
        for (int k = 0; k < kLevels; ++k) {
            if (!done) {
                if ((cnt >> k) & 1u) v = lvl[k] + v;
                else {
                    lvl[k] = v;
                    done = true;
                }
            }
        }
        ++cnt;
    }

    __device__ __forceinline__ float total() const {
        float acc = 0.0f;
        bool have = false;
#pragma unroll
        for (int k = 0; k < kLevels; ++k) {
            if ((cnt >> k) & 1u) {
                acc = have ? lvl[k] + acc : lvl[k];
                have = true;
            }
        }
        return acc;
    }
};

// one workgroup: S_b = tree over part[b][0, nch); out[0] = scale * tree over b of S_b.  Thread t owns rows [t R, (t + 1) R),
// R a power of two with 256 R >= nrows.
__global__ void __launch_bounds__(kBlock) k_tree_finish(const float* __restrict__ part, int64_t nrows, int nch, int64_t R,
                                                        float* __restrict__ row_sums, float scale, float* __restrict__ out) {
    __shared__ float lds4[4];
    TreeFold rows;
    const int64_t b0 = (int64_t)threadIdx.x * R;
    for (int64_t r = 0; r < R && b0 + r < nrows; ++r) {
        const float* __restrict__ p = part + (b0 + r) * (int64_t)nch;
        float S;
        if (nch == 1) S = p[0];
        else {
            TreeFold ch;
            for (int c = 0; c < nch; ++c) ch.push(p[c]);
            S = ch.total();
        }
        if (row_sums) row_sums[b0 + r] = S;
        rows.push(S);
    }
    TreePath path;
    const float tot = block_upsweep(rows.total(), path, lds4);
    if (threadIdx.x == 0) out[0] = scale * tot;
}

int64_t rows_per_thread(int64_t nrows) {
    int64_t R = 1;
    while (R * kBlock < nrows) R <<= 1;
    return R;
}

// ------------------------------------------------------------------------------------------------
// clip + adam + ema
// ------------------------------------------------------------------------------------------------
struct AdamArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    const float* gnorm2;
    int64_t n;
    float lr, b1, b2, eps, bc1, bc2, max_norm, decay;
    int ema_mode;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float& ema, const AdamArgs& a, float s) {
    g = g * s;
    m = a.b1 * m + (1.0f - a.b1) * g;
    v = a.b2 * v + (1.0f - a.b2) * (g * g);
    const float u = (m / a.bc1) / (fbsmi_sqrtf(v / a.bc2) + a.eps);
    p = p - a.lr * u;
    if (a.ema_mode == 1) ema = p;
    else if (a.ema_mode == 2) ema = a.decay * ema + (1.0f - a.decay) * p;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) k_adam_ema(AdamArgs a) {
    float s = 1.0f;
    if (a.gnorm2) {
        const float gn = fbsmi_sqrtf(a.gnorm2[0]);
        s = gn < a.max_norm ? 1.0f : a.max_norm / gn;
    }
    const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, nth = (int64_t)gridDim.x * kBlock;
    const int64_t n4 = VEC ? a.n / 4 : 0;
    for (int64_t i = tid; i < n4; i += nth) {
        float4 p = ((float4*)a.p)[i], m = ((float4*)a.m)[i], v = ((float4*)a.v)[i];
        const float4 g = ((const float4*)a.g)[i];
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.ema_mode == 2) e = ((float4*)a.ema)[i];
        adam_one(p.x, g.x, m.x, v.x, e.x, a, s);
        adam_one(p.y, g.y, m.y, v.y, e.y, a, s);
        adam_one(p.z, g.z, m.z, v.z, e.z, a, s);
        adam_one(p.w, g.w, m.w, v.w, e.w, a, s);
        ((float4*)a.p)[i] = p;
        ((float4*)a.m)[i] = m;
        ((float4*)a.v)[i] = v;
        if (a.ema_mode != 0) ((float4*)a.ema)[i] = e;
    }
    for (int64_t i = n4 * 4 + tid; i < a.n; i += nth) {   // the scalar tail (everything, without 16-byte alignment)
        float p = a.p[i], m = a.m[i], v = a.v[i], e = a.ema_mode == 2 ? a.ema[i] : 0.0f;
        adam_one(p, a.g[i], m, v, e, a, s);
        a.p[i] = p;
        a.m[i] = m;
        a.v[i] = v;
        if (a.ema_mode != 0) a.ema[i] = e;
    }
}

int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

}  // namespace fbsmi

using namespace fbsmi;

extern "C" {

int fbsmi_uniform_host(uint32_t k0, uint32_t k1, int64_t n, float* out_host) {
    FBSMI_NEED(n >= 0 && (n == 0 || out_host), "uniform_host: bad arguments");
    for (int64_t i = 0; i < n; ++i) out_host[i] = uniform_at(k0, k1, (uint64_t)n, (uint64_t)i);
    return FBSMI_OK;
}

int fbsmi_dsm_noise_batched(const float* data, const int32_t* idx, const uint32_t* keys, const float* F, const float* sq,
                            int64_t B, int64_t D, int out_dtype, void* xt, void* stream) {
    FBSMI_NEED(data && keys && F && sq && xt, "dsm_noise_batched: null pointer");
    FBSMI_NEED(B >= 1 && D >= 1, "dsm_noise_batched: B and D must be at least 1");
    FBSMI_NEED(D <= kMaxDraw, "dsm_noise_batched: a row exceeds 2^32 - 4 elements");
    FBSMI_NEED(out_dtype == 0 || out_dtype == 1, "dsm_noise_batched: out_dtype must be 0 or 1");
    const bool vec = D % 8 == 0 && aligned16(data) && aligned16(xt);
    const int64_t half = (D + 1) / 2, work = vec ? half / 4 : half;
    int64_t bpr = (work + kBlock - 1) / kBlock;
    if (bpr > kMaxRowGroups) bpr = kMaxRowGroups;
    FBSMI_NEED(B <= kMaxGrid / bpr, "dsm_noise_batched: too many rows for one grid");
    const unsigned grid = (unsigned)(B * bpr);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == 0) {
        if (vec) k_dsm_noise<0, true><<<grid, kBlock, 0, st>>>(data, idx, keys, F, sq, (uint64_t)D, (int)bpr, xt);
        else k_dsm_noise<0, false><<<grid, kBlock, 0, st>>>(data, idx, keys, F, sq, (uint64_t)D, (int)bpr, xt);
    } else {
        if (vec) k_dsm_noise<1, true><<<grid, kBlock, 0, st>>>(data, idx, keys, F, sq, (uint64_t)D, (int)bpr, xt);
        else k_dsm_noise<1, false><<<grid, kBlock, 0, st>>>(data, idx, keys, F, sq, (uint64_t)D, (int)bpr, xt);
    }
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

size_t fbsmi_dsm_loss_workspace_bytes(int64_t B, int64_t D) {
    if (B < 1 || D < 1 || D > kMaxDraw) return 0;
    return (size_t)B * (size_t)chunks_of(D) * sizeof(float);
}

int fbsmi_dsm_loss_batched(const void* net, int net_dtype, int mode, const uint32_t* keys, const float* xt, const float* data,
                           const int32_t* idx, const float* F, const float* sq, const float* gc, float inv, int64_t B,
                           int64_t D, void* dnet, float* row_sums, float* loss, void* workspace, void* stream) {
    FBSMI_NEED(net && sq && gc && dnet && loss && workspace, "dsm_loss_batched: null pointer");
    FBSMI_NEED(mode == 0 || mode == 1, "dsm_loss_batched: mode must be 0 (drawn) or 1 (stored)");
    FBSMI_NEED(net_dtype == 0 || net_dtype == 1, "dsm_loss_batched: net_dtype must be 0 or 1");
    FBSMI_NEED(mode == 1 || keys, "dsm_loss_batched: mode 0 needs keys");
    FBSMI_NEED(mode == 0 || (xt && data && F), "dsm_loss_batched: mode 1 needs xt, data and F");
    FBSMI_NEED(B >= 1 && D >= 1, "dsm_loss_batched: B and D must be at least 1");
    FBSMI_NEED(D <= kMaxDraw, "dsm_loss_batched: a row exceeds 2^32 - 4 elements");
    const int64_t nch = chunks_of(D);
    const int64_t wpr = nch < kMaxRowGroups ? nch : kMaxRowGroups;
    FBSMI_NEED(B <= kMaxGrid / wpr, "dsm_loss_batched: too many rows for one grid");
    const bool vec = D % 8 == 0 && aligned16(net) && aligned16(dnet) && (mode == 0 || (aligned16(xt) && aligned16(data)));
    DsmLossArgs a{net, keys, xt, data, idx, F, sq, gc, dnet, (float*)workspace, (uint64_t)D, (int)nch, (int)wpr};
    const unsigned grid = (unsigned)(B * wpr);
    hipStream_t st = (hipStream_t)stream;
#define FBSMI_DSM_LAUNCH(NETDT, MODE)                                           \
    do {                                                                        \
        if (vec) k_dsm_loss<NETDT, MODE, true><<<grid, kBlock, 0, st>>>(a);     \
        else k_dsm_loss<NETDT, MODE, false><<<grid, kBlock, 0, st>>>(a);        \
    } while (0)
    if (net_dtype == 0 && mode == 0) FBSMI_DSM_LAUNCH(0, 0);
    else if (net_dtype == 0) FBSMI_DSM_LAUNCH(0, 1);
    else if (mode == 0) FBSMI_DSM_LAUNCH(1, 0);
    else FBSMI_DSM_LAUNCH(1, 1);
#undef FBSMI_DSM_LAUNCH
    FBSMI_LAUNCH_CHECK();
    k_tree_finish<<<1, kBlock, 0, st>>>((const float*)workspace, B, (int)nch, rows_per_thread(B), row_sums, inv, loss);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

size_t fbsmi_sqnorm_workspace_bytes(int64_t n) { return n < 1 ? 0 : (size_t)chunks_of(n) * sizeof(float); }

int fbsmi_sqnorm(const float* x, int64_t n, float* out, void* workspace, void* stream) {
    FBSMI_NEED(x && out && workspace, "sqnorm: null pointer");
    FBSMI_NEED(n >= 1, "sqnorm: n must be at least 1");
    const int64_t nch = chunks_of(n);
    FBSMI_NEED(nch <= kMaxGrid, "sqnorm: the vector is too long");
    const unsigned grid = (unsigned)(nch < kMaxFlatGroups ? nch : kMaxFlatGroups);
    hipStream_t st = (hipStream_t)stream;
    if (aligned16(x)) k_sq_chunks<true><<<grid, kBlock, 0, st>>>(x, (uint64_t)n, nch, (float*)workspace);
    else k_sq_chunks<false><<<grid, kBlock, 0, st>>>(x, (uint64_t)n, nch, (float*)workspace);
    FBSMI_LAUNCH_CHECK();
    // the chunk roots are the rows of the finishing launch: one root each
    k_tree_finish<<<1, kBlock, 0, st>>>((const float*)workspace, nch, 1, rows_per_thread(nch), nullptr, 1.0f, out);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float b1, float b2,
                        float eps, float bc1, float bc2, const float* gnorm2, float max_norm, int ema_mode, float decay,
                        void* stream) {
    FBSMI_NEED(p && g && m && v, "adam_ema_step: null pointer");
    FBSMI_NEED(ema_mode >= 0 && ema_mode <= 2, "adam_ema_step: ema_mode must be 0, 1 or 2");
    FBSMI_NEED(ema_mode == 0 || ema, "adam_ema_step: ema_mode 1 and 2 need ema");
    FBSMI_NEED(n >= 1, "adam_ema_step: n must be at least 1");
    FBSMI_NEED(bc1 > 0.0f && bc2 > 0.0f, "adam_ema_step: the bias corrections must be positive");
    FBSMI_NEED(!gnorm2 || max_norm > 0.0f, "adam_ema_step: max_norm must be positive");
    AdamArgs a{p, g, m, v, ema, gnorm2, n, lr, b1, b2, eps, bc1, bc2, max_norm, decay, ema_mode};
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (ema_mode == 0 || aligned16(ema));
    int64_t groups = ((vec ? (n + 3) / 4 : n) + kBlock - 1) / kBlock;
    if (groups > kMaxFlatGroups) groups = kMaxFlatGroups;
    hipStream_t st = (hipStream_t)stream;
    if (vec) k_adam_ema<true><<<(unsigned)groups, kBlock, 0, st>>>(a);
    else k_adam_ema<false><<<(unsigned)groups, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

}  // extern "C"
