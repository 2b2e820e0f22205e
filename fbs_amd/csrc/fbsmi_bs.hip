// fbsmi_bs.hip -- fused backward simulation for the analytic (linear-Gaussian) model, batched over chains:
// bootstrap_backward_smoother (fbs/samplers/smc.py:91-112, mode 0) and backward_sampling_pass
// (fbs/samplers/csmc/csmc.py:167-227, mode 1).  The numeric specification is in include/fbsmi.h (fbsmi_lg_backsim_*).
//
// The recursion is T strictly serial steps, but the transition MEANS are a function of the stored path alone:
//   k_bs_mean   mean[t][r][i] for a chunk of time slices at once (all the O(n D du) arithmetic of the pass), ahead of the
//               serial steps that consume it; the workspace is `tch` time slices;
// a serial step is then a row sum over du, the normalisation and one search, in grid-wide stages:
//   lw    [pick of the step before: uniform, bisection, row copy] + log-weights + per-tile (max, sumexp)   [mode 1: max]
//   x     (mode 1) shift by the global max, add the stored log-weights, per-tile (max, sumexp)
//   norm  logsumexp from the tile pairs, w = exp(. - lse), per-tile sums of w
//   cdf   top tree over the tile sums, two-value descent: the canonical cumsum
// The pick is done by every workgroup of the next `lw` launch for itself (same cdf, same key, same answer), so it costs no
// launch of its own: 3 launches per step in mode 0, 4 in mode 1, plus one closing launch.  With one tile (n <= 256) a single
// workgroup per chain runs the same stages back to back, a workgroup barrier between them: one launch per chunk of steps.
// The chain is blockIdx.y.  gfx950 only.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"

namespace fbsmi {

constexpr int kBsMeanTile = 64;                  // slots per workgroup of k_bs_mean: one per lane
constexpr int kBsMeanRows = 4;                   // drift rows a wave accumulates together
constexpr int kBsMeanPitch = kBsMeanTile + 1;    // LDS pitch of a staged coordinate (odd: conflict-free both ways)
constexpr int kBsMaxD = 128;

struct BsDev {
    int n, du, dv, D, T, C, mode, nb, levels, lh, tch;
    float dt;
    const float* G;        // [T][D][D]
    const float* g;        // [T][D]
    const float* sd;       // [T]
    const float* lognorm;  // [T]
    const float** io;      // [0] path (C,T+1,n,du), [1] log_wss (C,T+1,n): the caller's arrays of this call
    uint32_t* keys;        // [C][2]
    uint32_t* kt;          // [C][T+1][2]: the key that picks time t
    float* vs;             // [C][T+1][dv]
    float* mean;           // [C][tch][du][n]
    float* lw;             // [C][n] log-weights (mode 1: gl)
    float* x;              // [C][n] mode 1: shifted log-weights
    float* w;              // [C][n]
    float* cdf;            // [C][n]
    float* pmax;           // [C][nb] per-tile max
    float* psum;           // [C][nb] per-tile sum of exp
    float* ptot;           // [C][nb] per-tile sum of w
    float* pgmax;          // [C][nb] mode 1: per-tile max of gl
    int32_t* sel;          // [C][T+1] picked slot per time
    float* traj;           // [C][T+1][du]
};

// one chain's slice of everything
struct BsChain {
    const float* path;
    const float* lwss;
    const uint32_t* kt;
    const float* vs;
    float *mean, *lw, *x, *w, *cdf, *pmax, *psum, *ptot, *pgmax, *traj;
    int32_t* sel;
};

__device__ __forceinline__ BsChain bs_chain(const BsDev& d, int c) {
    BsChain k;
    const size_t T1 = (size_t)d.T + 1;
    k.path = d.io[0] + (size_t)c * T1 * d.n * d.du;
    k.lwss = d.mode == 1 ? d.io[1] + (size_t)c * T1 * d.n : nullptr;
    k.kt = d.kt + (size_t)c * T1 * 2;
    k.vs = d.vs + (size_t)c * T1 * d.dv;
    k.mean = d.mean + (size_t)c * d.tch * d.du * d.n;
    k.lw = d.lw + (size_t)c * d.n;
    k.x = d.x + (size_t)c * d.n;
    k.w = d.w + (size_t)c * d.n;
    k.cdf = d.cdf + (size_t)c * d.n;
    k.pmax = d.pmax + (size_t)c * d.nb;
    k.psum = d.psum + (size_t)c * d.nb;
    k.ptot = d.ptot + (size_t)c * d.nb;
    k.pgmax = d.pgmax + (size_t)c * d.nb;
    k.traj = d.traj + (size_t)c * T1 * d.du;
    k.sel = d.sel + (size_t)c * T1;
    return k;
}

struct BsLds {
    float a[4], b[4], c[4], m[4];
    float x8[8];
    float bc[2];
    float heap[kHeapSize];
    float win[kBlock];
};

// the caller's arrays of this call (outside the captured graph: the graph's kernels find them here)
__global__ void k_bs_io(const float** io, const float* path, const float* log_wss) {
    if (threadIdx.x == 0) {
        io[0] = path;
        io[1] = log_wss;
    }
}

// keys.  mode 0: iT = randint(key, (), 0, n) with the parent key; keys = split(split(key, 2)[1], T)      smc.py:108-110
//        mode 1: keys = split(key, T + 1); keys[T] draws B_T, keys[s] draws time T-1-s                    csmc.py:194,201,214
__global__ void __launch_bounds__(kBlock) k_bs_keys(BsDev d) {
    const int c = blockIdx.y;
    const BsChain k = bs_chain(d, c);
    const uint32_t k0 = d.keys[2 * c], k1 = d.keys[2 * c + 1];
    uint32_t* kt = d.kt + (size_t)c * (d.T + 1) * 2;
    if (d.mode == 0) {
        uint32_t s0, s1;
        split_at(k0, k1, 2, 1, s0, s1);
        for (int s = threadIdx.x; s < d.T; s += kBlock) {
            const int t = d.T - 1 - s;
            split_at(s0, s1, d.T, s, kt[2 * t], kt[2 * t + 1]);
        }
        const int iT = randint_at(k0, k1, 1, 0, 0, d.n);
        if (threadIdx.x == 0) k.sel[d.T] = iT;
        const float* row = k.path + ((size_t)d.T * d.n + iT) * d.du;
        for (int r = threadIdx.x; r < d.du; r += kBlock) k.traj[(size_t)d.T * d.du + r] = row[r];
    } else {
        for (int s = threadIdx.x; s <= d.T; s += kBlock) {
            const int t = s == d.T ? d.T : d.T - 1 - s;
            split_at(k0, k1, d.T + 1, s, kt[2 * t], kt[2 * t + 1]);
        }
    }
}

// mean[tl][r][i] = path[t][i][r] + drift_r(path[t][i], vs[t]) * dt for t = t0 + tl (blockIdx.y), slots of tile blockIdx.x:
// a lane owns a slot, a wave owns drift rows (its G entries are wave-uniform: scalar operands), the tile's particle rows are
// staged in LDS coordinate-major.  The fma chain is the specification's: started at g[r], c ascending over (u, v).
__global__ void __launch_bounds__(kBlock) k_bs_mean(BsDev d, int t0) {
    __shared__ float zs[kBsMaxD * kBsMeanPitch];
    const int c = blockIdx.z, tl = blockIdx.y, t = t0 + tl;
    const BsChain k = bs_chain(d, c);
    const int p0 = blockIdx.x * kBsMeanTile;
    const float* slice = k.path + (size_t)t * d.n * d.du;
    for (int idx = threadIdx.x; idx < kBsMeanTile * d.du; idx += kBlock) {
        const int p = idx / d.du, cc = idx - p * d.du;
        const int gi = p0 + p < d.n ? p0 + p : d.n - 1;   // (clamped address, no predicated load)
        zs[cc * kBsMeanPitch + p] = slice[(size_t)gi * d.du + cc];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* Gt = d.G + (size_t)t * d.D * d.D;
    const float* gt = d.g + (size_t)t * d.D;
    const float* v = k.vs + (size_t)t * d.dv;
    float* out = k.mean + (size_t)tl * d.du * d.n;
    const int i = p0 + lane;
    for (int r0 = wave * kBsMeanRows; r0 < d.du; r0 += kWaves * kBsMeanRows) {
        float acc[kBsMeanRows];
        const float* Gr[kBsMeanRows];
#pragma unroll
        for (int j = 0; j < kBsMeanRows; ++j) {
            const int r = r0 + j < d.du ? r0 + j : d.du - 1;
            Gr[j] = Gt + (size_t)r * d.D;
            acc[j] = gt[r];
        }
        for (int cc = 0; cc < d.du; ++cc) {
            const float z = zs[cc * kBsMeanPitch + lane];
#pragma unroll
            for (int j = 0; j < kBsMeanRows; ++j) acc[j] = fbsmi_fmaf(Gr[j][cc], z, acc[j]);
        }
        for (int cc = 0; cc < d.dv; ++cc) {
            const float z = v[cc];
#pragma unroll
            for (int j = 0; j < kBsMeanRows; ++j) acc[j] = fbsmi_fmaf(Gr[j][d.du + cc], z, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kBsMeanRows; ++j) {
            const int r = r0 + j;
            if (r < d.du && i < d.n) out[(size_t)r * d.n + i] = zs[r * kBsMeanPitch + lane] + acc[j] * d.dt;
        }
    }
}

// ------------------------------------------------------------------------------------------
// the stages of a serial step, for tile b of one chain (every thread of the workgroup calls them)
// ------------------------------------------------------------------------------------------

// cat(kt[t], w) from the finished cdf: the picked slot, the same in every thread
__device__ __forceinline__ int bs_pick(const BsDev& d, const BsChain& k, BsLds& L, int t) {
    const float u = uniform_at(k.kt[2 * t], k.kt[2 * t + 1], 1, 0);
    const float q = k.cdf[d.n - 1] * (1.0f - u);
    if (threadIdx.x >= 1 && threadIdx.x < kHeapSize) L.heap[threadIdx.x] = k.cdf[heap_node_mid(threadIdx.x, d.n)];
    __syncthreads();
    const int B = bisect_uniform(k.cdf, d.n, d.levels, d.lh, L.heap, L.win, q);
    __syncthreads();
    return B;
}

// record the pick of time t: bs[t] and traj[t] = path[t][B]
__device__ __forceinline__ void bs_record(const BsDev& d, const BsChain& k, int t, int B) {
    const int Bc = B < d.n ? B : d.n - 1;
    if (threadIdx.x == 0) k.sel[t] = B;
    const float* row = k.path + ((size_t)t * d.n + Bc) * d.du;
    for (int r = threadIdx.x; r < d.du; r += kBlock) k.traj[(size_t)t * d.du + r] = row[r];
}

// lw_i = tlp(t, path[t+1][B], i) from the tabulated means of slot tl; tile partials
__device__ __forceinline__ void bs_stage_lw(const BsDev& d, const BsChain& k, BsLds& L, int b, int t, int tl, bool pick) {
    int B;
    if (pick) {
        B = bs_pick(d, k, L, t + 1);
        if (b == 0) bs_record(d, k, t + 1, B);
    } else {
        B = k.sel[t + 1];
    }
    const int Bc = B < d.n ? B : d.n - 1;
    const float* xrow = k.path + ((size_t)(t + 1) * d.n + Bc) * d.du;
    const int i = b * kBlock + threadIdx.x;
    const bool valid = i < d.n;
    const float* mp = k.mean + (size_t)tl * d.du * d.n + (valid ? i : d.n - 1);
    const float sd = d.sd[t], ln = d.lognorm[t];
    const float sd2 = sd * sd;
    float acc = 0.0f;
    for (int r = 0; r < d.du; ++r) {
        const float dlt = xrow[r] - mp[(size_t)r * d.n];
        const float lp = (ln + (dlt * dlt) / sd2) / -2.0f;
        acc = r == 0 ? lp : acc + lp;
    }
    if (valid) k.lw[i] = acc;
    const float l1[1] = {valid ? acc : -__builtin_inff()};
    if (d.mode == 0) {
        float m, s;
        block_lse_partial<1>(l1, L.a, L.b, m, s);
        if (threadIdx.x == 0) {
            k.pmax[b] = m;
            k.psum[b] = s;
        }
    } else {
        const float m = block_max(l1[0], L.m);
        if (threadIdx.x == 0) k.pgmax[b] = m;
    }
}

// mode 1: x_i = (gl_i - max(gl)) + log_wss[t][i]  (t == T: x = log_wss[T], the draw of B_T); tile partials
__device__ __forceinline__ void bs_stage_x(const BsDev& d, const BsChain& k, BsLds& L, int b, int t, bool has_gl) {
    const int i = b * kBlock + threadIdx.x;
    const bool valid = i < d.n;
    const int ic = valid ? i : d.n - 1;
    float xi = k.lwss[(size_t)t * d.n + ic];
    if (has_gl) {
        const float gmax = top_max(k.pgmax, d.nb, L.m);
        xi = (k.lw[ic] - gmax) + xi;
    }
    if (valid) k.x[i] = xi;
    const float l1[1] = {valid ? xi : -__builtin_inff()};
    float m, s;
    block_lse_partial<1>(l1, L.a, L.b, m, s);
    if (threadIdx.x == 0) {
        k.pmax[b] = m;
        k.psum[b] = s;
    }
}

// w_i = exp(src_i - lse(src)); per-tile sum of w
__device__ __forceinline__ void bs_stage_norm(const BsDev& d, const BsChain& k, BsLds& L, int b) {
    const int i = b * kBlock + threadIdx.x;
    const bool valid = i < d.n;
    const float* src = d.mode == 0 ? k.lw : k.x;
    const float l = src[valid ? i : d.n - 1];
    float c, Mraw;
    lse_from_partials(k.pmax, k.psum, d.nb, L.a, L.b, c, Mraw);
    const float w = valid ? fbsmi_expf(l - c) : 0.0f;
    if (valid) k.w[i] = w;
    float s1[1] = {w}, t1[1];
    TreePath p1[1];
    block_upsweep_n<1>(s1, p1, L.c, t1);
    if (threadIdx.x == 0) k.ptot[b] = t1[0];
}

// cdf = cumsum(w) in the canonical tree order: top tree over the tile sums, descent to the leaf
__device__ __forceinline__ void bs_stage_cdf(const BsDev& d, const BsChain& k, BsLds& L, int b) {
    const int i = b * kBlock + threadIdx.x;
    const bool valid = i < d.n;
    const float wl = k.w[valid ? i : d.n - 1];
    const float wv = valid ? wl : 0.0f;
    float pw[kTopItems];
    top_load(k.ptot, d.nb, pw);
    float s2[2] = {chunk_total<kTopItems>(pw), wv}, t2[2];
    TreePath p2[2];
    block_upsweep_n<2>(s2, p2, L.x8, t2);
    float P, E;
    top_leaf(pw, p2[0], t2[0], b, L.bc, P, E);
    block_descend(P, E, p2[1]);
    if (valid) k.cdf[i] = E;
}

// ---- several tiles: one launch per stage --------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_bs_lw(BsDev d, int t, int tl, int pick) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    bs_stage_lw(d, k, L, blockIdx.x, t, tl, pick != 0);
}

__global__ void __launch_bounds__(kBlock) k_bs_x(BsDev d, int t, int has_gl) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    bs_stage_x(d, k, L, blockIdx.x, t, has_gl != 0);
}

__global__ void __launch_bounds__(kBlock) k_bs_norm(BsDev d) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    bs_stage_norm(d, k, L, blockIdx.x);
}

__global__ void __launch_bounds__(kBlock) k_bs_cdf(BsDev d) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    bs_stage_cdf(d, k, L, blockIdx.x);
}

// the pick of time 0, which no later step makes
__global__ void __launch_bounds__(kBlock) k_bs_last(BsDev d) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    const int B = bs_pick(d, k, L, 0);
    bs_record(d, k, 0, B);
}

// ---- one tile (n <= 256): one workgroup per chain runs steps t_hi .. t_lo of a chunk in one launch ---------------
// (a stage reads what the stage before wrote to global memory from the same workgroup: a barrier orders them)
__device__ __forceinline__ void bs_stage_sync() {
    __threadfence_block();
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) k_bs_pass1(BsDev d, int t_hi, int t_lo) {
    __shared__ BsLds L;
    const BsChain k = bs_chain(d, blockIdx.y);
    if (d.mode == 1 && t_hi == d.T - 1) {   // B_T ~ Cat(exp(log_wss[T] - lse))
        bs_stage_x(d, k, L, 0, d.T, false);
        bs_stage_sync();
        bs_stage_norm(d, k, L, 0);
        bs_stage_sync();
        bs_stage_cdf(d, k, L, 0);
        bs_stage_sync();
    }
    for (int t = t_hi; t >= t_lo; --t) {
        bs_stage_lw(d, k, L, 0, t, t - t_lo, !(d.mode == 0 && t == d.T - 1));
        bs_stage_sync();
        if (d.mode == 1) {
            bs_stage_x(d, k, L, 0, t, true);
            bs_stage_sync();
        }
        bs_stage_norm(d, k, L, 0);
        bs_stage_sync();
        bs_stage_cdf(d, k, L, 0);
        bs_stage_sync();
    }
    if (t_lo == 0) {
        const int B = bs_pick(d, k, L, 0);
        bs_record(d, k, 0, B);
    }
}

}  // namespace fbsmi

using namespace fbsmi;

struct fbsmi_lg_backsim {
    BsDev d{};
    void* slab = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraphExec_t graph = nullptr;
};

namespace {

// the launch sequence of one pass on stream st (after k_bs_io)
int enqueue_backsim(fbsmi_lg_backsim* h, hipStream_t st) {
    const BsDev& d = h->d;
    const dim3 gchain(1, d.C), gtile(d.nb, d.C);
    const bool one_tile = d.n <= kBlock;
    k_bs_keys<<<gchain, kBlock, 0, st>>>(d);
    if (d.mode == 1 && !one_tile) {
        k_bs_x<<<gtile, kBlock, 0, st>>>(d, d.T, 0);
        k_bs_norm<<<gtile, kBlock, 0, st>>>(d);
        k_bs_cdf<<<gtile, kBlock, 0, st>>>(d);
    }
    for (int t_hi = d.T - 1; t_hi >= 0; t_hi -= d.tch) {
        const int t_lo = t_hi - d.tch + 1 > 0 ? t_hi - d.tch + 1 : 0;
        const dim3 gmean((d.n + kBsMeanTile - 1) / kBsMeanTile, t_hi - t_lo + 1, d.C);
        k_bs_mean<<<gmean, kBlock, 0, st>>>(d, t_lo);
        if (one_tile) {
            k_bs_pass1<<<gchain, kBlock, 0, st>>>(d, t_hi, t_lo);
            continue;
        }
        for (int t = t_hi; t >= t_lo; --t) {
            k_bs_lw<<<gtile, kBlock, 0, st>>>(d, t, t - t_lo, !(d.mode == 0 && t == d.T - 1));
            if (d.mode == 1) k_bs_x<<<gtile, kBlock, 0, st>>>(d, t, 1);
            k_bs_norm<<<gtile, kBlock, 0, st>>>(d);
            k_bs_cdf<<<gtile, kBlock, 0, st>>>(d);
        }
    }
    if (!one_tile) k_bs_last<<<gchain, kBlock, 0, st>>>(d);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? FBSMI_OK : fail(FBSMI_ERR_HIP, std::string("backsim launch: ") + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int fbsmi_lg_backsim_create(const fbsmi_lg_model* m, int32_t nslots, int mode, int32_t nchains, fbsmi_lg_backsim** out) {
    if (!out || !m || mode < 0 || mode > 1 || nchains < 1 || nchains > 65535)
        return fail(FBSMI_ERR_ARG, "lg_backsim_create: mode must be 0 (smoother) | 1 (backward sampling), 1 <= nchains <= 65535");
    *out = nullptr;
    if (m->du < 1 || m->dv < 0 || m->T < 1 || !m->G || !m->g || !m->sd || !m->lognorm)
        return fail(FBSMI_ERR_ARG, "lg_backsim_create: bad model");
    if (nslots < 1 || nslots > 131072 || fbsmi_tile_items(nslots) != 1)
        return fail(FBSMI_ERR_UNSUPPORTED, "lg_backsim_create: 1 <= nslots <= 131072");
    if (m->du > kBsMaxD || m->dv > kBsMaxD) return fail(FBSMI_ERR_UNSUPPORTED, "lg_backsim_create: max(du, dv) <= 128");
    fbsmi_lg_backsim* h = new (std::nothrow) fbsmi_lg_backsim();
    if (!h) return fail(FBSMI_ERR_ARG, "out of host memory");
    BsDev& d = h->d;
    d.n = nslots;
    d.du = m->du;
    d.dv = m->dv;
    d.D = m->du + m->dv;
    d.T = m->T;
    d.C = nchains;
    d.mode = mode;
    d.nb = (nslots + kBlock - 1) / kBlock;
    d.levels = bisect_levels(nslots);
    d.lh = d.levels < kHeapLevels ? d.levels : kHeapLevels;
    d.dt = m->dt;
    d.G = m->G;
    d.g = m->g;
    d.sd = m->sd;
    d.lognorm = m->lognorm;
    // time slices of means per chunk: up to 16, within 256 MB
    const size_t slice = sizeof(float) * (size_t)d.C * d.du * d.n;
    size_t tch = ((size_t)256 << 20) / slice;
    tch = tch < 1 ? 1 : (tch > 16 ? 16 : tch);
    d.tch = (int)(tch > (size_t)d.T ? (size_t)d.T : tch);

    const size_t C = d.C, T1 = (size_t)d.T + 1, n = d.n, nb = d.nb;
    size_t bytes = 0;
    auto take = [&](size_t b) {
        const size_t off = bytes;
        bytes += (b + 255) & ~(size_t)255;
        return off;
    };
    const size_t o_io = take(2 * sizeof(float*)), o_keys = take(C * 2 * 4), o_kt = take(C * T1 * 2 * 4),
                 o_vs = take(C * T1 * (d.dv ? d.dv : 1) * 4), o_mean = take(C * d.tch * d.du * n * 4), o_lw = take(C * n * 4),
                 o_x = take(C * n * 4), o_w = take(C * n * 4), o_cdf = take(C * n * 4), o_pmax = take(C * nb * 4),
                 o_psum = take(C * nb * 4), o_ptot = take(C * nb * 4), o_pgmax = take(C * nb * 4), o_sel = take(C * T1 * 4),
                 o_traj = take(C * T1 * d.du * 4);
    auto bail = [&](hipError_t e, const char* what) {
        const int rc = fail(FBSMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        fbsmi_lg_backsim_destroy(h);
        return rc;
    };
    hipError_t e = hipMalloc(&h->slab, bytes);
    if (e != hipSuccess) return bail(e, "hipMalloc");
    if ((e = hipMemset(h->slab, 0, bytes)) != hipSuccess) return bail(e, "hipMemset");
    char* base = (char*)h->slab;
    d.io = (const float**)(base + o_io);
    d.keys = (uint32_t*)(base + o_keys);
    d.kt = (uint32_t*)(base + o_kt);
    d.vs = (float*)(base + o_vs);
    d.mean = (float*)(base + o_mean);
    d.lw = (float*)(base + o_lw);
    d.x = (float*)(base + o_x);
    d.w = (float*)(base + o_w);
    d.cdf = (float*)(base + o_cdf);
    d.pmax = (float*)(base + o_pmax);
    d.psum = (float*)(base + o_psum);
    d.ptot = (float*)(base + o_ptot);
    d.pgmax = (float*)(base + o_pgmax);
    d.sel = (int32_t*)(base + o_sel);
    d.traj = (float*)(base + o_traj);
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    *out = h;
    return FBSMI_OK;
}

void fbsmi_lg_backsim_destroy(fbsmi_lg_backsim* h) {
    if (!h) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->graph) (void)hipGraphExecDestroy(h->graph);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->slab) (void)hipFree(h->slab);
    delete h;
}

int fbsmi_lg_backsim_run(fbsmi_lg_backsim* h, const uint32_t* keys, const float* vs, const float* path, const float* log_wss,
                         float* traj, int32_t* bs, int use_graph, void* stream) {
    if (!h || !keys || !path || !traj || (!vs && h->d.dv > 0)) return fail(FBSMI_ERR_ARG, "lg_backsim_run: null input");
    const BsDev& d = h->d;
    if (d.mode == 1 && !log_wss) return fail(FBSMI_ERR_ARG, "lg_backsim_run: backward sampling needs log_wss");
    hipStream_t ust = (hipStream_t)stream, st = h->stream;
    const size_t C = d.C, T1 = (size_t)d.T + 1;
    // the pass runs on the handle's stream, after what the caller's stream holds so far; what the caller queues next waits
    FBSMI_HIP_TRY(hipEventRecord(h->ev_in, ust));
    FBSMI_HIP_TRY(hipStreamWaitEvent(st, h->ev_in, 0));
    FBSMI_HIP_TRY(hipMemcpyAsync(d.keys, keys, C * 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (d.dv > 0) FBSMI_HIP_TRY(hipMemcpyAsync(d.vs, vs, C * T1 * d.dv * sizeof(float), hipMemcpyDeviceToDevice, st));
    k_bs_io<<<1, 64, 0, st>>>(d.io, path, log_wss);
    if (int rc = launch_captured(h->graph, st, use_graph != 0, [&] { return enqueue_backsim(h, st); })) return rc;
    FBSMI_HIP_TRY(hipMemcpyAsync(traj, d.traj, C * T1 * d.du * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (bs) FBSMI_HIP_TRY(hipMemcpyAsync(bs, d.sel, C * T1 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    FBSMI_HIP_TRY(hipEventRecord(h->ev_out, st));
    FBSMI_HIP_TRY(hipStreamWaitEvent(ust, h->ev_out, 0));
    return FBSMI_OK;
}

}  // extern "C"
