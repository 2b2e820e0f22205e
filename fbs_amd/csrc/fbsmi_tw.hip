// fbsmi_tw.hip -- fused twisted SMC (fbs/samplers/smc.py:261-309; Algorithm 1 of arXiv 2306.17775) for the analytic
// Gaussian model of experiments/toy/gp_twisted.py, batched over independent runs (include/fbsmi.h, fbsmi_tw_*).
//
// For a Gaussian prior the twisting function is a Gaussian density of an affine map of the particle, so its gradient is
// affine and one SMC step is two matrix products and three row-summed Gaussian log-densities:
//   product A  [C_j; R_j] (2d x d) on the gathered ancestors: rows < d give the proposal mean m and the new particle x
//              (in-kernel normal draw), rows >= d the transition mean;
//   product B  R_j (d x d) on the new particles: the row terms of the twist.
// Both run on the f32 matrix cores (v_mfma_f32_16x16x4_f32 accumulates as an ascending fmaf chain, bit for bit:
// tools/mfmatest.hip), one workgroup = 32 slots x 32 rows, tiles in LDS in the plane layout of fbsmi_lg.hip's wide_pos.
// Run b of the batch is blockIdx.y.  Launches per step:
//   N <= 256 : k_tw_gemm<0> (stratified / systematic search + A) -> k_tw_gemm<1> (B) -> k_tw_lw (row sums in row order,
//              lw, and -- the ensemble being one logsumexp tile -- the normalisation and the canonical cumsum) : 3
//   N  > 256 : k_tw_norm -> k_tw_cdf -> k_tw_gemm<0> -> k_tw_gemm<1> -> k_tw_lw (tile (max, sumexp) pairs)      : 5
// A whole run (keys, init draw, twist_0, T steps, final normalisation, optional choice) is one captured hipGraph.
#include <math.h>

#include <new>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"

using namespace fbsmi;

namespace {

constexpr int kTwTile = 32;
typedef float mfma_f4 __attribute__((ext_vector_type(4)));

struct TwDev {
    int d, T, N, B, nb, levels, systematic, select;
    float dt, obs_var, lognorm_obs;
    const float *R, *r, *C, *c, *sd, *lognorm, *m_ref, *Lt, *y;   // the caller's tables (fbsmi_tw_model)
    uint32_t* keys;     // [B][2]          the call's keys
    uint32_t* keytab;   // [B][4 + 4 T]    key_init, key_select, then per step (key_resampling, key_prop)
    float *x0, *x1;     // [B][N][d]       particles, ping-pong: step k reads x(k & 1)
    float *mb, *tb, *pb;   // [B][N][d]    proposal means, transition means, twist terms
    float *lps0, *lps1;    // [B][N]       log_ps, ping-pong like the particles
    float *tl, *pl;        // [B][N]       the last step's transition / proposal log-densities (views)
    float *lw, *logw, *cdf;   // [B][N]
    float *bmax, *bsumexp, *bsumw;   // [B][nb]
    int32_t* anc;       // [B][N]
    int32_t* As;        // [B][T][N], nullable
    float* samples;     // [B][d]
};

__device__ __forceinline__ TwDev run_view(TwDev d, int b) {
    const size_t n = (size_t)b * d.N, nd = n * d.d, t = (size_t)b * d.nb;
    d.keys += 2 * b;
    d.keytab += (size_t)b * (4 + 4 * d.T);
    d.x0 += nd; d.x1 += nd; d.mb += nd; d.tb += nd; d.pb += nd;
    d.lps0 += n; d.lps1 += n; d.tl += n; d.pl += n; d.lw += n; d.logw += n; d.cdf += n; d.anc += n;
    d.bmax += t; d.bsumexp += t; d.bsumw += t;
    if (d.As) d.As += (size_t)b * d.T * d.N;
    d.samples += (size_t)b * d.d;
    return d;
}

// jax.scipy.stats.norm.logpdf with s2 = scale^2 and ln = log(2 pi scale^2)  (norm_logpdf of fbsmi_lg.hip)
__device__ __forceinline__ float tw_nlp(float x, float loc, float s2, float ln) {
    const float dlt = x - loc;
    return (ln + (dlt * dlt) / s2) / -2.0f;
}

// wide_pos / wide_plane_row of fbsmi_lg.hip: element (row i, column c) of a 32-row LDS tile, S floats per plane row
__device__ __forceinline__ int tw_pos(int i, int c, int S) { return ((c & 3) * kTwTile + i) * S + (c >> 2); }
inline int tw_plane_row(int Kp) { return ((Kp / 4) & 4) ? Kp / 4 : Kp / 4 + 4; }

// key (, key_select) = split(key) when a sample is asked for (gp_twisted.py:134); key_init, key_filter = split(key);
// keys = split(key_filter, T); key_resampling, key_prop = split(keys[k])  (smc.py:298-299,281)
__global__ void __launch_bounds__(kBlock) k_tw_keys(TwDev dd) {
    const TwDev d = run_view(dd, blockIdx.y);
    uint32_t f0 = d.keys[0], f1 = d.keys[1], s0 = 0, s1 = 0;
    if (d.select) {
        const uint32_t k0 = f0, k1 = f1;
        split_at(k0, k1, 2, 0, f0, f1);
        split_at(k0, k1, 2, 1, s0, s1);
    }
    uint32_t i0, i1, g0, g1;
    split_at(f0, f1, 2, 0, i0, i1);
    split_at(f0, f1, 2, 1, g0, g1);
    if (threadIdx.x == 0) {
        d.keytab[0] = i0; d.keytab[1] = i1; d.keytab[2] = s0; d.keytab[3] = s1;
    }
    for (int k = threadIdx.x; k < d.T; k += kBlock) {
        uint32_t q0, q1;
        split_at(g0, g1, d.T, k, q0, q1);
        uint32_t* kt = d.keytab + 4 + 4 * k;
        split_at(q0, q1, 2, 0, kt[0], kt[1]);   // key_resampling
        split_at(q0, q1, 2, 1, kt[2], kt[3]);   // key_prop
    }
}

// init_sampler (gp_twisted.py:107-110): x[n][i] = m_ref[i] + sum_c z[n][c] Lt[c][i], products and sums rounded one by one
// in ascending c (the form of k_pm_u0).  A workgroup owns 256 consecutive elements of x; the normals of the particles it
// touches are drawn once into LDS.
__global__ void __launch_bounds__(kBlock) k_tw_init(TwDev dd) {
    const TwDev d = run_view(dd, blockIdx.y);
    __shared__ float zs[kBlock + 2 * 128];
    const int D = d.d;
    const size_t total = (size_t)d.N * D;
    const size_t e0 = (size_t)blockIdx.x * kBlock;
    const size_t elast = e0 + kBlock - 1 < total - 1 ? e0 + kBlock - 1 : total - 1;
    const size_t z0 = (e0 / D) * D, z1 = (elast / D + 1) * D;   // the normals [z0, z1) of whole particles: at most 256 + 2 D - 2
    for (size_t q = z0 + threadIdx.x; q < z1; q += kBlock) zs[q - z0] = normal_at(d.keytab[0], d.keytab[1], total, q);
    __syncthreads();
    const size_t e = e0 + threadIdx.x;
    if (e >= total) return;
    const int i = (int)(e % D);
    const float* z = zs + ((e / D) * D - z0);
    float acc = z[0] * d.Lt[i];
    for (int c = 1; c < D; ++c) acc = acc + z[c] * d.Lt[(size_t)c * D + i];
    d.x0[e] = d.m_ref[i] + acc;
}

// The drift product and what hangs on it.  nrt = row tiles of this launch, Kp = d rounded up to 16, S = tw_plane_row(Kp).
// MODE 0 (product A, step k, time point j = k + 1): the ancestors of the workgroup's 32 slots are searched in the cdf
//   (resampling.py:43-51), their rows gathered from x(k & 1); rows < d: m = xp + drift(C_j, c_j, xp) dt, x = m + sd_j z;
//   rows >= d: tm = xp + drift(R_j, r_j, xp) dt.
// MODE 1 (product B, time point j): the slots' own rows of x(which); rows < d: the terms of twist_j.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_tw_gemm(TwDev dd, int j, int k, int which, int nrt, int Kp, int S) {
    const TwDev d = run_view(dd, blockIdx.y);
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ int ancS[kTwTile];
    float* Gs = dyn;                     // 32 rows of the stacked matrix
    float* Zs = dyn + 4 * kTwTile * S;   // 32 gathered slots
    const int N = d.N, D = d.d, rows = MODE == 0 ? 2 * D : D;
    const int ts = blockIdx.x / nrt, tr = blockIdx.x - ts * nrt;
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const float* __restrict__ xs = which ? d.x1 : d.x0;
    float* __restrict__ xn = which ? d.x0 : d.x1;
    const uint32_t* kt = d.keytab + 4 + 4 * k;
    if (MODE == 0) {
        if (t < kTwTile) {
            const int mj = kTwTile * ts + t;
            int a = -1;
            if (mj < N) {
                const float uu = d.systematic ? uniform_at(kt[0], kt[1], 1, 0) : uniform_at(kt[0], kt[1], (uint64_t)N, (uint64_t)mj);
                const float q = ((float)mj + uu) / (float)N;
                a = searchsorted_left(d.cdf, N, d.levels, q);
                a = a < 0 ? 0 : (a > N - 1 ? N - 1 : a);
                if (tr == 0) {
                    d.anc[mj] = a;
                    if (d.As) d.As[(size_t)k * N + mj] = a;
                }
            }
            ancS[t] = a;
        }
    } else if (t < kTwTile) {
        const int mj = kTwTile * ts + t;
        ancS[t] = mj < N ? mj : -1;
    }
    __syncthreads();
    // wave w stages rows / slots w, w + 4, ... of the two tiles; lane l columns l and l + 64
    constexpr int kRows = kTwTile / kWaves;
#pragma unroll
    for (int q = 0; q < kRows * 2; ++q) {
        const int i = wave + kWaves * (q >> 1), c = lane + 64 * (q & 1);
        if (c < Kp) {
            const int r = kTwTile * tr + i, a = ancS[i];
            float gv = 0.0f, zv = 0.0f;
            if (r < rows && c < D) {
                const float* M = (MODE == 0 && r < D) ? d.C + ((size_t)j * D + r) * D : d.R + ((size_t)j * D + (r - (MODE == 0 ? D : 0))) * D;
                gv = M[c];
            }
            if (a >= 0 && c < D) zv = xs[(size_t)a * D + c];
            const int pos = tw_pos(i, c, S);
            Gs[pos] = gv;
            Zs[pos] = zv;
        }
    }
    // accumulator geometry of v_mfma_f32_16x16x4_f32: wave = (row half ar, slot half ac); register v of a lane holds
    // (row 4 (lane / 16) + v, slot lane % 16) of the 16 x 16 block
    const int ar = wave >> 1, ac = wave & 1;
    const int row0 = kTwTile * tr + 16 * ar + 4 * (lane >> 4);
    const int jloc = 16 * ac + (lane & 15);
    const int mo = kTwTile * ts + jloc;
    mfma_f4 acc;
#pragma unroll
    for (int vv = 0; vv < 4; ++vv) {
        const int r = row0 + vv;
        float b = 0.0f;
        if (r < rows) b = (MODE == 0 && r < D) ? d.c[(size_t)j * D + r] : d.r[(size_t)j * D + (r - (MODE == 0 ? D : 0))];
        acc[vv] = b;
    }
    float xi[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (MODE == 0 && kTwTile * tr < D) {   // four independent Threefry + erf_inv chains, under the staging loads
        uint32_t bits[4];
#pragma unroll
        for (int vv = 0; vv < 4; ++vv) {
            const int r = row0 + vv;
            const bool ok = r < D && mo < N;
            bits[vv] = random_bits_at(kt[2], kt[3], (uint64_t)N * D, ok ? (uint64_t)mo * D + r : 0ull);
        }
#pragma unroll
        for (int vv = 0; vv < 4; ++vv) xi[vv] = normal_from_bits(bits[vv]);
    }
    __syncthreads();
    // acc = bias_r, then acc = fma(M[r][c], z[c], acc) for c ascending, on the matrix cores
    {
        const float4* ga = reinterpret_cast<const float4*>(Gs + tw_pos(16 * ar + (lane & 15), lane >> 4, S));
        const float4* zb = reinterpret_cast<const float4*>(Zs + tw_pos(jloc, lane >> 4, S));
        const int nq = kTwTile * tr + 16 * ar < rows ? Kp >> 4 : 0;
        float4 a0 = ga[0], b0 = zb[0];
#pragma unroll 1
        for (int q4 = 0; q4 < nq; q4 += 2) {
            const int q1 = q4 + 1 < nq ? q4 + 1 : q4, q2 = q4 + 2 < nq ? q4 + 2 : q4;
            const float4 a1 = ga[q1], b1 = zb[q1];
            __builtin_amdgcn_sched_barrier(0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (q4 + 1 < nq) {
                a0 = ga[q2];
                b0 = zb[q2];
                __builtin_amdgcn_sched_barrier(0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if (mo >= N) return;
    if (MODE == 0) {
        const float sd = d.sd[j];
#pragma unroll
        for (int vv = 0; vv < 4; ++vv) {
            const int r = row0 + vv;
            if (r < D) {
                const float m = Zs[tw_pos(jloc, r, S)] + acc[vv] * d.dt;
                d.mb[(size_t)mo * D + r] = m;
                xn[(size_t)mo * D + r] = m + sd * xi[vv];
            } else if (r < rows) {
                const int i = r - D;
                d.tb[(size_t)mo * D + i] = Zs[tw_pos(jloc, i, S)] + acc[vv] * d.dt;
            }
        }
    } else {
#pragma unroll
        for (int vv = 0; vv < 4; ++vv) {
            const int r = row0 + vv;
            if (r < D) {
                const float loc = Zs[tw_pos(jloc, r, S)] + acc[vv] * d.dt;
                d.pb[(size_t)mo * D + r] = tw_nlp(d.y[r], loc, d.obs_var, d.lognorm_obs);
            }
        }
    }
}

// Row sums in row order (acc = term_0, then acc + term_i), lw and the tile's (max, sumexp) pair.  INIT: lw = log_ps = twist_0(x).
// Otherwise (step k, time point j = k + 1) lw = ((tl + log_ps) - pl) - log_ps_prev[ancestor].  One tile (N <= 256): the
// normalisation (lse = log(sumexp) + max', exactly what the two-level combine gives for one tile) and the canonical cumsum
// of the weights follow here, call for call the arithmetic of k_tw_norm -> k_tw_cdf.
template <bool INIT>
__global__ void __launch_bounds__(kBlock) k_tw_lw(TwDev dd, int j, int k) {
    const TwDev d = run_view(dd, blockIdx.y);
    __shared__ float xch[3][4];
    const int N = d.N, D = d.d;
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const bool live = n < N;
    const int which = INIT ? 0 : (k & 1);   // the step read x(which) and wrote the other one
    const float* __restrict__ x = INIT ? d.x0 : (which ? d.x0 : d.x1);
    const float* __restrict__ lpp = which ? d.lps1 : d.lps0;
    float* __restrict__ lpn = INIT ? d.lps0 : (which ? d.lps0 : d.lps1);
    float l = 0.0f;
    if (live) {
        const float* __restrict__ pb = d.pb + (size_t)n * D;
        float lp = pb[0];
        for (int i = 1; i < D; ++i) lp = lp + pb[i];
        l = lp;
        if (!INIT) {
            const float sd = d.sd[j], sd2 = sd * sd, ln = d.lognorm[j];
            const float* __restrict__ xr = x + (size_t)n * D;
            const float* __restrict__ mb = d.mb + (size_t)n * D;
            const float* __restrict__ tb = d.tb + (size_t)n * D;
            float tl = tw_nlp(xr[0], tb[0], sd2, ln), pl = tw_nlp(xr[0], mb[0], sd2, ln);
            for (int i = 1; i < D; ++i) {
                tl = tl + tw_nlp(xr[i], tb[i], sd2, ln);
                pl = pl + tw_nlp(xr[i], mb[i], sd2, ln);
            }
            d.tl[n] = tl;
            d.pl[n] = pl;
            l = ((tl + lp) - pl) - lpp[d.anc[n]];
        }
        lpn[n] = lp;
        d.lw[n] = l;
    }
    float lv[1] = {live ? l : -__builtin_inff()};
    float Mraw, sx;
    block_lse_partial<1>(lv, xch[0], xch[1], Mraw, sx);
    if (d.nb > 1) {
        if (threadIdx.x == 0) {
            d.bmax[blockIdx.x] = Mraw;
            d.bsumexp[blockIdx.x] = sx;
        }
        return;
    }
    const float c = fbsmi_logf(sx) + finite_or_zero_f(Mraw);
    float w = 0.0f;
    if (live) {
        const float lg = l - c;
        d.logw[n] = lg;
        w = fbsmi_expf(lg);
    }
    float s1[1] = {w}, t1[1];
    TreePath p1[1];
    block_upsweep_n<1>(s1, p1, xch[2], t1);
    float P = 0.0f, E = t1[0], cc[1];
    const float xw1[1] = {w};
    block_descend(P, E, p1[0]);
    chunk_scan<1>(xw1, P, E, cc);
    if (live) d.cdf[n] = cc[0];
}

// N > 256: log_ws = lw - logsumexp(lw) from the tile pairs, w = exp(log_ws), the tile's sum of w
__global__ void __launch_bounds__(kBlock) k_tw_norm(TwDev dd) {
    const TwDev d = run_view(dd, blockIdx.y);
    __shared__ float xch[3][4];
    const int n = blockIdx.x * kBlock + threadIdx.x;
    const float l = n < d.N ? d.lw[n] : 0.0f;
    float c, Mraw;
    lse_from_partials(d.bmax, d.bsumexp, d.nb, xch[0], xch[1], c, Mraw);
    float w = 0.0f;
    if (n < d.N) {
        const float lg = l - c;
        d.logw[n] = lg;
        w = fbsmi_expf(lg);
    }
    float s1[1] = {w}, t1[1];
    TreePath p1[1];
    block_upsweep_n<1>(s1, p1, xch[2], t1);
    if (threadIdx.x == 0) d.bsumw[blockIdx.x] = t1[0];
}

// N > 256: canonical cumsum of w = exp(log_ws) (k_lg_cdf<1, 2> of fbsmi_lg.hip: top tree over the tile sums, then the tile)
__global__ void __launch_bounds__(kBlock) k_tw_cdf(TwDev dd) {
    const TwDev d = run_view(dd, blockIdx.y);
    __shared__ float xch[2][4];
    __shared__ float bc[2];
    const int b = blockIdx.x;
    const int n = b * kBlock + threadIdx.x;
    const float wv[1] = {n < d.N ? fbsmi_expf(d.logw[n]) : 0.0f};
    float pw[kTopItems];
    top_load(d.bsumw, d.nb, pw);
    float c[1];
    float s2[2] = {chunk_total<kTopItems>(pw), wv[0]}, t2[2];
    TreePath p2[2];
    block_upsweep_n<2>(s2, p2, xch[0], t2);
    float P, E;
    top_leaf(pw, p2[0], t2[0], b, bc, P, E);
    block_descend(P, E, p2[1]);
    chunk_scan<1>(wv, P, E, c);
    if (n < d.N) d.cdf[n] = c[0];
}

// jax.random.choice(key_select, N, (), p = exp(log_ws)) and the chosen row (gp_twisted.py:141)
__global__ void __launch_bounds__(kBlock) k_tw_choice(TwDev dd, int which) {
    const TwDev d = run_view(dd, blockIdx.y);
    const float u = uniform_at(d.keytab[2], d.keytab[3], 1, 0);
    int a = searchsorted_left(d.cdf, d.N, d.levels, d.cdf[d.N - 1] * (1.0f - u));
    a = a < 0 ? 0 : (a > d.N - 1 ? d.N - 1 : a);
    const float* x = which ? d.x1 : d.x0;
    for (int i = threadIdx.x; i < d.d; i += kBlock) d.samples[i] = x[(size_t)a * d.d + i];
}

}  // namespace

struct fbsmi_tw {
    TwDev d{};
    void* pool = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraphExec_t graph[2] = {nullptr, nullptr};   // [select]
};

namespace {

int tw_enqueue(fbsmi_tw* h, hipStream_t st) {
    const TwDev& d = h->d;
    const int Kp = (d.d + 15) & ~15, S = tw_plane_row(Kp);
    const size_t lds = sizeof(float) * 2 * 4 * kTwTile * (size_t)S;
    const int nst = (d.N + kTwTile - 1) / kTwTile;
    const int nrtA = (2 * d.d + kTwTile - 1) / kTwTile, nrtB = (d.d + kTwTile - 1) / kTwTile;
    const dim3 gtile(d.nb, d.B), gA(nst * nrtA, d.B), gB(nst * nrtB, d.B);
    const dim3 ginit((unsigned)(((size_t)d.N * d.d + kBlock - 1) / kBlock), d.B);
    k_tw_keys<<<dim3(1, d.B), kBlock, 0, st>>>(d);
    k_tw_init<<<ginit, kBlock, 0, st>>>(d);
    k_tw_gemm<1><<<gB, kBlock, lds, st>>>(d, 0, 0, 0, nrtB, Kp, S);
    k_tw_lw<true><<<gtile, kBlock, 0, st>>>(d, 0, 0);
    for (int k = 0; k < d.T; ++k) {
        if (d.nb > 1) {
            k_tw_norm<<<gtile, kBlock, 0, st>>>(d);
            k_tw_cdf<<<gtile, kBlock, 0, st>>>(d);
        }
        k_tw_gemm<0><<<gA, kBlock, lds, st>>>(d, k + 1, k, k & 1, nrtA, Kp, S);
        k_tw_gemm<1><<<gB, kBlock, lds, st>>>(d, k + 1, k, (k & 1) ^ 1, nrtB, Kp, S);
        k_tw_lw<false><<<gtile, kBlock, 0, st>>>(d, k + 1, k);
    }
    if (d.nb > 1) {
        k_tw_norm<<<gtile, kBlock, 0, st>>>(d);
        if (d.select) k_tw_cdf<<<gtile, kBlock, 0, st>>>(d);
    }
    if (d.select) k_tw_choice<<<dim3(1, d.B), kBlock, 0, st>>>(d, d.T & 1);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FBSMI_ERR_HIP, std::string("twisted smc launch: ") + hipGetErrorString(e));
    return FBSMI_OK;
}

}  // namespace

extern "C" {

int fbsmi_tw_create(const fbsmi_tw_model* m, int32_t nparticles, int resampling, int32_t nruns, int store_ancestors,
                    fbsmi_tw** out) {
    if (!out || !m || resampling < 0 || resampling > 1 || nruns < 1 || m->T < 1)
        return fail(FBSMI_ERR_ARG, "tw_create: need a model, T >= 1, nruns >= 1 and resampling 0 (stratified) | 1 (systematic)");
    if (!m->R || !m->r || !m->C || !m->c || !m->sd || !m->lognorm || !m->m_ref || !m->Lt || !m->y)
        return fail(FBSMI_ERR_ARG, "tw_create: null table");
    if (nruns > 65535)   // run b of the batch is blockIdx.y of every launch
        return fail(FBSMI_ERR_UNSUPPORTED, "tw_create: the fused twisted SMC takes 1 <= nruns <= 65535 (one grid row per run)");
    if (m->d < 1 || m->d > 128 || nparticles < 1 || nparticles > 131072)
        return fail(FBSMI_ERR_UNSUPPORTED, "tw_create: the fused twisted SMC takes 1 <= d <= 128 and 1 <= nparticles <= 131072");
    fbsmi_tw* h = new (std::nothrow) fbsmi_tw();
    if (!h) return fail(FBSMI_ERR_ARG, "out of host memory");
    TwDev& d = h->d;
    d.d = m->d; d.T = m->T; d.N = nparticles; d.B = nruns;
    d.nb = (nparticles + kBlock - 1) / kBlock;
    d.levels = bisect_levels(nparticles);
    d.systematic = resampling;
    d.dt = m->dt; d.obs_var = m->obs_var; d.lognorm_obs = m->lognorm_obs;
    d.R = m->R; d.r = m->r; d.C = m->C; d.c = m->c; d.sd = m->sd; d.lognorm = m->lognorm;
    d.m_ref = m->m_ref; d.Lt = m->Lt; d.y = m->y;
    const size_t B = nruns, N = nparticles, D = m->d, T = m->T, nb = d.nb;
    // one allocation, carved in 256-byte steps
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_keys = take(B * 2 * 4), o_ktab = take(B * (4 + 4 * T) * 4);
    const size_t o_x0 = take(B * N * D * 4), o_x1 = take(B * N * D * 4), o_mb = take(B * N * D * 4), o_tb = take(B * N * D * 4),
                 o_pb = take(B * N * D * 4);
    const size_t o_l0 = take(B * N * 4), o_l1 = take(B * N * 4), o_tl = take(B * N * 4), o_pl = take(B * N * 4), o_lw = take(B * N * 4),
                 o_lg = take(B * N * 4), o_cdf = take(B * N * 4), o_anc = take(B * N * 4);
    const size_t o_bm = take(B * nb * 4), o_bs = take(B * nb * 4), o_bw = take(B * nb * 4), o_smp = take(B * D * 4);
    const size_t o_As = store_ancestors ? take(B * T * N * 4) : 0;
    auto bail = [&](hipError_t e, const char* what) {
        const int rc = fail(FBSMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        fbsmi_tw_destroy(h);
        return rc;
    };
    hipError_t e;
    if ((e = hipMalloc(&h->pool, off)) != hipSuccess) return bail(e, "tw_create: hipMalloc");
    if ((e = hipMemset(h->pool, 0, off)) != hipSuccess) return bail(e, "tw_create: hipMemset");
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "tw_create: hipStreamCreate");
    if ((e = hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming)) != hipSuccess) return bail(e, "tw_create: hipEventCreate");
    if ((e = hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming)) != hipSuccess) return bail(e, "tw_create: hipEventCreate");
    char* p = (char*)h->pool;
    d.keys = (uint32_t*)(p + o_keys); d.keytab = (uint32_t*)(p + o_ktab);
    d.x0 = (float*)(p + o_x0); d.x1 = (float*)(p + o_x1); d.mb = (float*)(p + o_mb); d.tb = (float*)(p + o_tb); d.pb = (float*)(p + o_pb);
    d.lps0 = (float*)(p + o_l0); d.lps1 = (float*)(p + o_l1); d.tl = (float*)(p + o_tl); d.pl = (float*)(p + o_pl);
    d.lw = (float*)(p + o_lw); d.logw = (float*)(p + o_lg); d.cdf = (float*)(p + o_cdf); d.anc = (int32_t*)(p + o_anc);
    d.bmax = (float*)(p + o_bm); d.bsumexp = (float*)(p + o_bs); d.bsumw = (float*)(p + o_bw); d.samples = (float*)(p + o_smp);
    d.As = store_ancestors ? (int32_t*)(p + o_As) : nullptr;
    *out = h;
    return FBSMI_OK;
}

void fbsmi_tw_destroy(fbsmi_tw* h) {
    if (!h) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& g : h->graph)
        if (g) (void)hipGraphExecDestroy(g);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->pool) (void)hipFree(h->pool);
    delete h;
}

int fbsmi_tw_run(fbsmi_tw* h, const uint32_t* keys, int select, float* xs, float* log_ws, float* samples, int use_graph,
                 void* stream) {
    if (!h || !keys) return fail(FBSMI_ERR_ARG, "tw_run: null input");
    if (samples && !select) return fail(FBSMI_ERR_ARG, "tw_run: samples are only drawn with select != 0");
    TwDev& d = h->d;
    d.select = select ? 1 : 0;
    hipStream_t ust = (hipStream_t)stream, st = h->stream;
    const size_t B = d.B, N = d.N, D = d.d;
    FBSMI_HIP_TRY(hipEventRecord(h->ev_in, ust));
    FBSMI_HIP_TRY(hipStreamWaitEvent(st, h->ev_in, 0));
    FBSMI_HIP_TRY(hipMemcpyAsync(d.keys, keys, B * 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (!use_graph) {
        if (int rc = tw_enqueue(h, st)) return rc;
    } else {
        hipGraphExec_t& slot = h->graph[d.select];
        if (!slot) {
            hipGraph_t g = nullptr;
            FBSMI_HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
            int rc = tw_enqueue(h, st);
            hipError_t e = hipStreamEndCapture(st, &g);
            if (!rc && e != hipSuccess) rc = fail(FBSMI_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            if (!rc && (e = hipGraphInstantiate(&slot, g, nullptr, nullptr, 0)) != hipSuccess)
                rc = fail(FBSMI_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
            if (g) (void)hipGraphDestroy(g);
            if (rc) return rc;
        }
        FBSMI_HIP_TRY(hipGraphLaunch(slot, st));
    }
    const float* xT = (d.T & 1) ? d.x1 : d.x0;
    if (xs) FBSMI_HIP_TRY(hipMemcpyAsync(xs, xT, B * N * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (log_ws) FBSMI_HIP_TRY(hipMemcpyAsync(log_ws, d.logw, B * N * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (samples) FBSMI_HIP_TRY(hipMemcpyAsync(samples, d.samples, B * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    FBSMI_HIP_TRY(hipEventRecord(h->ev_out, st));
    FBSMI_HIP_TRY(hipStreamWaitEvent(ust, h->ev_out, 0));
    return FBSMI_OK;
}

int fbsmi_tw_view(fbsmi_tw* h, int which, void* dst, int64_t* count, void* stream) {
    if (!h) return fail(FBSMI_ERR_ARG, "tw_view: null handle");
    const TwDev& d = h->d;
    const size_t B = d.B, N = d.N, D = d.d, T = d.T;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = d.As; n = B * T * N; break;                           // ancestors of every step, int32
        case 1: src = (d.T & 1) ? d.lps1 : d.lps0; n = B * N; break;        // log_ps of the last step
        case 2: src = d.tl; n = B * N; break;                               // transition log-density of the last step
        case 3: src = d.pl; n = B * N; break;                               // proposal log-density of the last step
        case 4: src = (d.T & 1) ? d.x0 : d.x1; n = B * N * D; break;        // the particles before the last step
        case 5: src = d.anc; n = B * N; break;                              // ancestors of the last step, int32
        default: return fail(FBSMI_ERR_ARG, "tw_view: which must be 0..5");
    }
    if (!src) return fail(FBSMI_ERR_ARG, "tw_view: the handle was created without store_ancestors");
    if (count) *count = (int64_t)n;
    if (!dst) return FBSMI_OK;
    hipStream_t ust = (hipStream_t)stream;
    FBSMI_HIP_TRY(hipEventRecord(h->ev_in, ust));
    FBSMI_HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_in, 0));
    FBSMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, h->stream));
    FBSMI_HIP_TRY(hipEventRecord(h->ev_out, h->stream));
    FBSMI_HIP_TRY(hipStreamWaitEvent(ust, h->ev_out, 0));
    return FBSMI_OK;
}

}  // extern "C"
