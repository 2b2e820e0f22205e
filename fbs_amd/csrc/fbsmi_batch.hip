// fbsmi_batch.hip -- the closure tier's sampler operations for B independent ensembles that advance in lockstep (the test
// images of one run, the chains of one image): one launch per operation for all of them.
//
//   fbsmi_normalise_batched     row b = fbsmi_normalise on lw[b]
//   fbsmi_cond_killing_batched  row b = fbsmi_cond_resample(kind 1, keys[b], w[b], i[b], j[b], conditional)
//   fbsmi_em_concat_batched     ensemble b = fbsmi_em_concat
//   fbsmi_em_finish_batched     ensemble b = fbsmi_em_finish with n_total = n, row0 = 0, net_A = NULL
//   fbsmi_resample_batched      row b = fbsmi_resample(kind 0 stratified / 1 systematic, w[b], keys[b])
//   fbsmi_em_propose_batched    ensemble b = fbsmi_em_finish with A = net_A = A[b], n_total = n, row0 = 0, proposal only
//   fbsmi_em_csgm_step_batched  trajectory b = one step of fbs_amd/csgm.py: fbsmi_em_update, then the next network input
//   fbsmi_normal_batched        row b = fbsmi_normal(keys[b], n)
//   fbsmi_categorical_batched   row b = fbsmi_categorical(keys[b], w[b])
//   fbsmi_linear_path_batched   ensemble b = fbsmi_linear_path on normal(keys[b], (T, D)), written unpacked and in either order
//   fbsmi_em_fwd_step_batched   ensemble b = fbsmi_em_update on its own image, the path point written unpacked
//   fbsmi_force_move_batched    entry b = fbsmi_force_move(keys[b], w[b], k[b])
//   fbsmi_randint_batched       row b = fbsmi_randint(keys[b], n, lo, hi)
//   fbsmi_backscan_batched      ensemble b = backward_scanning_pass: normalise, categorical, back-trace, row gather
//   fbsmi_affine_em_path_batched  ensemble b = fbsmi_affine_em_path on its own keys, target and start, in either order
//   fbsmi_em_translp_batched    ensemble b = fbsmi_em_transition_logpdf on its own particles, network rows and target
//   fbsmi_backsim_pick_batched  ensemble b = one step of backward simulation: reweight, normalise, categorical, row copy
//
// each bit for bit, and the step of the image twisted SMC (whole-image particles; fbs_amd/twisted.py
// make_image_twisted_batched), which has no single-ensemble kernel to equal: its arithmetic is specified in include/fbsmi.h
//
//   fbsmi_tw_img_gather_batched     the resampled particles (the autograd leaf) and their previous twist values
//   fbsmi_tw_img_twist_batched      lp = the twisting log-density from the network output; optionally the step's weights
//   fbsmi_tw_img_cotangent_batched  the output cotangent of the network's vector-Jacobian product
//   fbsmi_tw_img_propose_batched    the twisted proposal with its in-kernel draw, and both row-summed log-densities
//
// An ensemble has 1 <= n <= 1024 rows, so everything the single-ensemble entry points spread over
// several launches and a workspace in memory -- the two-level logsumexp, the canonical-tree CDFs, the searches, the draws --
// fits ONE workgroup per ensemble and its LDS.  The trees are built in place in LDS the way k_top_scan (fbsmi_prims.hip)
// builds the top-level tree: an up-sweep over the element index, zero padded to a power of two, then the two-value descent
// of fbsmi_device.h per element.  Padding with zeros and the number of levels above the data do not change a bit (0 + x is
// exact), so the result is the tree fbsmi_cumsum / fbsmi_sum / fbsmi_logsumexp define whatever their tiling was.
//
// The two image kernels are plain: a workgroup per particle row, a thread per element.  The step they belong to spends
// its time in the network; the dispatch variants of fbsmi_em.hip are not repeated here.  gfx950 only.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"

namespace fbsmi {

namespace {

constexpr int kMaxRows = 1024;          // rows of one ensemble: one thread each
constexpr int kLseTile = 256;           // fbsmi_tile(n) for n <= 131072 (include/fbsmi_math.h)
constexpr int kMaxSeg = 4096;           // 256-element segments of an observed part: dv <= 2^20

// In-place up-sweep of the canonical tree over a[0, np), np a power of two, up to blocks of `top` elements: afterwards
// a[q * s + s - 1] is the tree sum of the aligned block q of s elements, for every power of two s <= top.  Every thread of
// the workgroup calls it; it starts and ends with a barrier.
__device__ __forceinline__ void lds_upsweep(float* a, int np, int top) {
    for (int d = 1; d < top; d <<= 1) {
        __syncthreads();
        for (int i = threadIdx.x; i < np / (2 * d); i += blockDim.x) {
            const int r = (i + 1) * 2 * d - 1;
            a[r] = a[r - d] + a[r];
        }
    }
    __syncthreads();
}

// scan value of element e from the up-swept tree (the E of its leaf)
__device__ __forceinline__ float lds_scan_at(const float* a, int np, int e) {
    float P = 0.0f, E = a[np - 1];
    int pos = 0;
    for (int d = np >> 1; d >= 1; d >>= 1) {
        const float t = P + a[pos + d - 1];
        if (e & d) {
            P = t;
            pos += d;
        } else {
            E = t;
        }
    }
    return E;
}

// ------------------------------------------------------------------------------------------------
// normalise: blockDim.x = np = next_pow2(n) (at least 64), thread e owns element e
// ------------------------------------------------------------------------------------------------
// the logsumexp of one row, l = this thread's element (-inf beyond n); tr (np floats) and smax (np / 64) are scratch.
// Every thread of the workgroup calls it and gets the same value; tr and smax may be reused after the next barrier.
__device__ __forceinline__ float lds_row_lse(float l, int n, int np, float* tr, float* smax) {
    const int e = threadIdx.x;
    const float mw = wave_max(l);
    if ((e & 63) == 0) smax[e >> 6] = mw;
    __syncthreads();
    // per-tile maxima of the two-level logsumexp: tile q = elements [256 q, 256 q + 256)
    const int tile = np < kLseTile ? np : kLseTile, wpt = tile >> 6 ? tile >> 6 : 1;
    const int ntile = np / tile, nb = (n + kLseTile - 1) / kLseTile;
    float mt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float m = -__builtin_inff();
        for (int w = 0; w < wpt; ++w)
            if (q < ntile) m = fmaxf(m, smax[q * wpt + w]);
        mt[q] = m;
    }
    const int myq = e / tile;
    float mine = mt[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) mine = myq == q ? mt[q] : mine;
    tr[e] = fbsmi_expf(l - finite_or_zero(mine));   // exp(-inf - m') = 0 beyond n: the zero padding
    lds_upsweep(tr, np, tile);
    const float Mp = finite_or_zero(fmaxf(fmaxf(mt[0], mt[1]), fmaxf(mt[2], mt[3])));
    float a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        a[q] = q < nb ? tr[(q < ntile ? q : 0) * tile + tile - 1] * fbsmi_expf(finite_or_zero(mt[q]) - Mp) : 0.0f;
    const float s01 = a[0] + a[1], s23 = a[2] + a[3];
    const float tot = s01 + s23;
    return fbsmi_logf(tot) + Mp;
}

__global__ void __launch_bounds__(kMaxRows) k_normalise_b(const float* __restrict__ lw, int n, int np, int log_space,
                                                          float* __restrict__ out, float* __restrict__ out_lse) {
    __shared__ float tr[kMaxRows];
    __shared__ float smax[kMaxRows / 64];
    const int b = blockIdx.x, e = threadIdx.x;
    const float l = e < n ? lw[(int64_t)b * n + e] : -__builtin_inff();
    const float lse = lds_row_lse(l, n, np, tr, smax);
    if (e == 0 && out_lse) out_lse[b] = lse;
    if (e < n) {
        const float v = l - lse;
        out[(int64_t)b * n + e] = log_space ? v : fbsmi_expf(v);
    }
}

// ------------------------------------------------------------------------------------------------
// conditional killing (csmc/resamplings.py:40-88; k_killing_finish and fbsmi_cond_resample in fbsmi_prims.hip)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMaxRows) k_cond_killing_b(const uint32_t* __restrict__ keys, const float* __restrict__ w,
                                                             const int32_t* __restrict__ iref, const int32_t* __restrict__ jref,
                                                             int n, int np, int32_t* __restrict__ idx) {
    __shared__ float sw[kMaxRows], tr[kMaxRows], cdf[kMaxRows], cdfJ[kMaxRows];
    __shared__ float smax[kMaxRows / 64];
    __shared__ int s_shift;
    const int b = blockIdx.x, e = threadIdx.x;
    const int32_t i_ref = iref[b], j_ref = jref[b];
    const float we = e < n ? w[(int64_t)b * n + e] : 0.0f;
    sw[e] = we;
    const float mw = wave_max(e < n ? we : -__builtin_inff());
    if ((e & 63) == 0) smax[e >> 6] = mw;
    __syncthreads();
    float w_max = -__builtin_inff();
    for (int q = 0; q < (np >> 6); ++q) w_max = fmaxf(w_max, smax[q]);
    // J_prob = (1 - w / w_max) / n with [i] = 0; its total gives J_prob[i] = max(1 - total, 0)
    const float jp = e < n ? (1.0f - we / w_max) / (float)n : 0.0f;
    tr[e] = e == i_ref ? 0.0f : jp;
    lds_upsweep(tr, np, np);
    const float J_i = fmaxf(1.0f - tr[np - 1], 0.0f);
    __syncthreads();
    tr[e] = (e == i_ref && e < n) ? J_i : jp;
    lds_upsweep(tr, np, np);
    cdfJ[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    tr[e] = we;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    const int levels = bisect_levels(n);
    // the three sub-keys of split(key, 3): kill test, redraw, rotation
    const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
    uint32_t a0, a1, b0, b1, c0, c1;
    split_at(k0, k1, 3, 0, a0, a1);
    split_at(k0, k1, 3, 1, b0, b1);
    if (e == 0) {
        split_at(k0, k1, 3, 2, c0, c1);
        const float u3 = uniform_at(c0, c1, 1, 0);
        const int32_t J = searchsorted_left(cdfJ, n, levels, cdfJ[n - 1] * (1.0f - u3));
        long long s = ((long long)j_ref - J) % n;
        if (s < 0) s += n;
        s_shift = (int)s;
    }
    __syncthreads();
    if (e < n) {
        int32_t src = e - s_shift;
        if (src < 0) src += n;
        const float ws = sw[src];
        const float u1 = uniform_at(a0, a1, (uint64_t)n, (uint64_t)src);
        int32_t a = src;
        if (u1 * w_max >= ws) {
            const float u2 = uniform_at(b0, b1, (uint64_t)n, (uint64_t)src);
            a = searchsorted_left(cdf, n, levels, cdf[n - 1] * (1.0f - u2));
        }
        if (e == j_ref) a = i_ref;
        idx[(int64_t)b * n + e] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// stratified / systematic resampling (resampling.py:43-58; fbsmi_resample and k_strat_search in fbsmi_prims.hip)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMaxRows) k_resample_b(const uint32_t* __restrict__ keys, const float* __restrict__ w,
                                                         int n, int np, int systematic, int32_t* __restrict__ idx) {
    __shared__ float tr[kMaxRows], cdf[kMaxRows];
    const int b = blockIdx.x, e = threadIdx.x;
    tr[e] = e < n ? w[(int64_t)b * n + e] : 0.0f;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    if (e < n) {
        const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
        const float u = systematic ? uniform_at(k0, k1, 1, 0) : uniform_at(k0, k1, (uint64_t)n, (uint64_t)e);
        const float q = ((float)e + u) / (float)n;
        int32_t k = searchsorted_left(cdf, n, bisect_levels(n), q);
        k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
        idx[(int64_t)b * n + e] = k;
    }
}

// ------------------------------------------------------------------------------------------------
// the image step: one workgroup of kBlock threads per particle row of the flat (B * n) axis
// ------------------------------------------------------------------------------------------------
struct BatchArgs {
    const float* us;
    const int32_t* A;
    const void* net;
    const float* v;
    const float* v_prev;
    const uint32_t* keys;
    const int32_t* pin_row;
    const float* pin_value;
    float* us_new;
    float* lw;
    const int32_t* u_off;
    const int32_t* v_off;
    const int32_t* role;
    void* img;
    int32_t du, dv, nmasks, n;
    float cx, cs, dt, sd;
    int32_t net_by_A;   // the network's output row is the ancestor's (b * n + A[b][r]), not the slot's (b * n + r)
};

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) { return fbsmi_u2f((uint32_t)h << 16); }

// round to nearest even; NaN stays NaN
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
    const uint32_t u = fbsmi_f2u(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int NETDT>
__device__ __forceinline__ float net_value(const void* net, int64_t at) {
    if (NETDT == 0) return ((const float*)net)[at];
    return bf16_bits_to_f32(((const unsigned short*)net)[at]);
}

template <int MODE>
__device__ __forceinline__ float reverse_drift(float cx, float cs, float x, float s) {
    if (MODE == 1) return s;
    const float t1 = cx * x, t2 = cs * s;
    return t1 + t2;
}

// the ancestor of row r of ensemble b, kept inside the ensemble whatever the index array holds
__device__ __forceinline__ int64_t source_row(const BatchArgs& a, int b, int r) {
    if (!a.A) return r;
    const int32_t s = a.A[(int64_t)b * a.n + r];
    return s < 0 ? 0 : (s > a.n - 1 ? a.n - 1 : s);
}

template <int OUTDT>
__global__ void __launch_bounds__(kBlock) k_em_concat_b(const BatchArgs a) {
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n), r = (int)(row - (int64_t)b * a.n);
    const int D = a.du + a.dv;
    const int32_t* __restrict__ role = a.role + (a.nmasks == 1 ? 0 : (int64_t)b * D);
    const float* __restrict__ x = a.us + ((int64_t)b * a.n + source_row(a, b, r)) * a.du;
    const float* __restrict__ vp = a.v_prev + (int64_t)b * a.dv;
    for (int e = threadIdx.x; e < D; e += kBlock) {
        const int o = role[e];
        const float xv = o >= 0 ? x[o] : vp[~o];
        if (OUTDT == 0) ((float*)a.img)[row * D + e] = xv;
        else ((unsigned short*)a.img)[row * D + e] = f32_to_bf16_bits(xv);
    }
}

template <int NETDT, int MODE>
__global__ void __launch_bounds__(kBlock) k_em_finish_b(const BatchArgs a) {
    __shared__ float seg[kMaxSeg];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n), r = (int)(row - (int64_t)b * a.n);
    const int du = a.du, dv = a.dv, D = du + dv;
    const int mb = a.nmasks == 1 ? 0 : b;
    const int64_t src = (int64_t)b * a.n + source_row(a, b, r);
    const int64_t net_row = (a.net_by_A ? src : row) * D;
    if (a.us_new) {
        // us_new[r] = (x + drift * dt) + sd * z, z = row r of normal(keys[b], (n, du)); the pinned row takes its value
        const int32_t* __restrict__ u_off = a.u_off + (int64_t)mb * du;
        const float* __restrict__ x = a.us + src * du;
        float* __restrict__ y = a.us_new + row * du;
        const uint32_t k0 = a.keys[2 * b], k1 = a.keys[2 * b + 1];
        const uint64_t ntot = (uint64_t)a.n * (uint64_t)du;
        const bool pinned = a.pin_row && a.pin_row[b] == r;
        for (int p = threadIdx.x; p < du; p += kBlock) {
            float out;
            if (pinned) {
                out = a.pin_value[(int64_t)b * du + p];
            } else {
                const float xv = x[p];
                const float s = net_value<NETDT>(a.net, net_row + u_off[p]);
                const float z = normal_from_bits(random_bits_at(k0, k1, ntot, (uint64_t)r * du + p));
                const float d = reverse_drift<MODE>(a.cx, a.cs, xv, s);
                const float m = xv + d * a.dt;
                const float nz = a.sd * z;
                out = m + nz;
            }
            y[p] = out;
        }
    }
    if (a.lw) {
        // lw[r] = tree-sum_j ( log(2 pi sd^2) + (v[j] - (v_prev[j] + drift_j * dt))^2 / sd^2 ) / -2 over the index bits of j:
        // four elements in the thread, six levels in the wave, the 256-element segment sums in LDS
        const int32_t* __restrict__ v_off = a.v_off + (int64_t)mb * dv;
        const float* __restrict__ v = a.v + (int64_t)b * dv;
        const float* __restrict__ vp = a.v_prev + (int64_t)b * dv;
        const int nseg = (dv + 255) >> 8;
        const int nsp = next_pow2(nseg > 1 ? nseg : 1);
        const float var = a.sd * a.sd;
        const float lognorm = fbsmi_logf(6.2831855f * var);
        for (int i = threadIdx.x; i < nsp; i += kBlock) seg[i] = 0.0f;
        __syncthreads();
        for (int s0 = 0; s0 < dv; s0 += 4 * kBlock) {   // uniform trip count: every wave takes part in every round
            const int j0 = s0 + (int)threadIdx.x * 4;
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                t[k] = 0.0f;
                if (j0 + k < dv) {
                    const float sv = net_value<NETDT>(a.net, net_row + v_off[j0 + k]);
                    const float bv = vp[j0 + k];
                    const float dr = reverse_drift<MODE>(a.cx, a.cs, bv, sv);
                    const float m = bv + dr * a.dt;
                    const float df = v[j0 + k] - m;
                    const float sq = df * df;
                    const float q = sq / var;
                    t[k] = (lognorm + q) * -0.5f;
                }
            }
            const float s01 = t[0] + t[1], s23 = t[2] + t[3];
            TreePath path;
            const float sum = wave_upsweep(s01 + s23, path);
            const int sg = (s0 >> 8) + ((int)threadIdx.x >> 6);
            if ((threadIdx.x & 63) == 0 && sg < nseg) seg[sg] = sum;
        }
        lds_upsweep(seg, nsp, nsp);
        if (threadIdx.x == 0) a.lw[row] = seg[nsp - 1];
    }
}

// ------------------------------------------------------------------------------------------------
// the image CSGM step (fbs_amd/csgm.py): one workgroup per trajectory, threads stride over the image positions.  `role`
// is a bijection between positions and (u, v) elements, so ONE pass does the Euler-Maruyama update of step k (unobserved
// positions: us -> us_new, noise = element noff + o of normal(keys[b], (ntot,))) and writes the network input of step
// k + 1 (the updated value there, F * y0 + sq * normal(est_keys[b], (dv,)) at the observed positions).  A thread touches
// only its own element: no barrier, no LDS, and us_new may be us.  The network read net[b * D + e] is coalesced
// (u_off[role[e]] == e).  BatchArgs: v_prev = y0, keys = the scan keys, sd = c; n is unused (a trajectory is one row).
// ------------------------------------------------------------------------------------------------
template <int NETDT, int OUTDT>
__global__ void __launch_bounds__(kBlock) k_em_csgm_step_b(const BatchArgs a, const uint32_t* __restrict__ est_keys, float F,
                                                           float sq, uint64_t ntot, uint64_t noff) {
    const int b = blockIdx.x;
    const int du = a.du, dv = a.dv, D = du + dv;
    const int32_t* __restrict__ role = a.role + (a.nmasks == 1 ? 0 : (int64_t)b * D);
    const float* x = a.us + (int64_t)b * du;
    float* y = a.us_new ? a.us_new + (int64_t)b * du : nullptr;
    const bool update = a.net != nullptr, image = a.img != nullptr;
    const uint32_t s0 = a.keys[2 * b], s1 = a.keys[2 * b + 1], e0 = est_keys[2 * b], e1 = est_keys[2 * b + 1];
    for (int e = threadIdx.x; e < D; e += kBlock) {
        const int r = role[e];
        const bool unobs = r >= 0;
        // the element inside its part whatever the table holds
        int o = unobs ? r : ~r;
        const int last = (unobs ? du : dv) - 1;
        o = o > last ? last : o;
        if (o < 0 || !(unobs ? (update || image) : image)) continue;   // dv == 0, or nothing to do at this position
        // one draw per position, from the trajectory's scan key or the step's re-noising key: both kinds of position go
        // through the same instructions, so a wave that holds both does not run the generator twice
        float z = 0.0f;
        if (unobs ? update : true)
            z = normal_from_bits(random_bits_at(unobs ? s0 : e0, unobs ? s1 : e1, unobs ? ntot : (uint64_t)dv,
                                                unobs ? noff + (uint64_t)o : (uint64_t)o));
        float out;
        if (unobs) {
            out = x[o];
            if (update) {
                const float s = net_value<NETDT>(a.net, (int64_t)b * D + e);
                const float d = reverse_drift<0>(a.cx, a.cs, out, s);
                const float m = out + d * a.dt;
                const float nz = a.sd * z;
                out = m + nz;
                y[o] = out;
            }
        } else {
            const float t1 = F * a.v_prev[(int64_t)b * dv + o], t2 = sq * z;
            out = t1 + t2;
        }
        if (image) {
            if (OUTDT == 0) ((float*)a.img)[(int64_t)b * D + e] = out;
            else ((unsigned short*)a.img)[(int64_t)b * D + e] = f32_to_bf16_bits(out);
        }
    }
}

// row b of out (B, n) = normal(keys[b], (n,)): k_random<2> of fbsmi_prims.hip (one Threefry call per pair of elements
// (n + 1) / 2 apart) with the key read per row -- that kernel takes ONE key by value, so it cannot serve B of them.
// `bpr` workgroups per row.
__global__ void __launch_bounds__(kBlock) k_normal_b(const uint32_t* __restrict__ keys, uint64_t n, int bpr,
                                                     float* __restrict__ out) {
    const int64_t b = blockIdx.x / bpr;
    const int q = (int)(blockIdx.x - b * bpr);
    const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
    float* __restrict__ o = out + b * (int64_t)n;
    const uint64_t half = (n + 1) >> 1;
    for (uint64_t i = (uint64_t)q * kBlock + threadIdx.x; i < half; i += (uint64_t)bpr * kBlock) {
        const uint64_t j = i + half;
        uint32_t lo, hi;
        random_bits_pair_padded(k0, k1, n, i, lo, hi);
        o[i] = normal_from_bits(lo);
        if (j < n) o[j] = normal_from_bits(hi);
    }
}

// ------------------------------------------------------------------------------------------------
// image twisted SMC (fbs_amd/twisted.py make_image_twisted_batched; the arithmetic is specified in include/fbsmi.h):
// particles are whole images, X (B * n, D) in image order; one workgroup per particle row, threads stride over the
// elements, four consecutive elements per thread and round.  The head of the twisting function -- the Gaussian likelihood
// of the observed pixels under the one-step denoising estimate den = x + (cx x + cs s) dt -- and its derivative with
// respect to den are closed forms here; only the network's own vector-Jacobian product stays with autograd.
// ------------------------------------------------------------------------------------------------
struct TwArgs {
    const float* X;
    const void* net;
    const float* vjp;
    const float* y;
    const uint32_t* keys;
    const float* tl_in;
    const float* pl_in;
    const float* lpg;
    float* out;        // ct (cotangent) or X_new (propose)
    void* out2;        // propose: the copy of X_new in the network's input dtype
    float* lp;
    float* lw;
    float* tl;
    float* pl;
    const int32_t* v_off;
    const int32_t* role;
    int32_t du, dv, nmasks, n;
    float cx, cs, dt, sd, var_y;
};

// den = x + rd * dt with rd = (cx * x) + (cs * s), every operation rounded separately
__device__ __forceinline__ float tw_den(const TwArgs& a, float x, float s, float& rd) {
    rd = reverse_drift<0>(a.cx, a.cs, x, s);
    const float p = rd * a.dt;
    return x + p;
}

// nlp(v, m, var) = (log(2 pi var) + (v - m)^2 / var) / -2 with lognorm = log(2 pi var) given
__device__ __forceinline__ float tw_nlp(float v, float m, float var, float lognorm) {
    const float df = v - m;
    const float sq = df * df;
    const float q = sq / var;
    return (lognorm + q) * -0.5f;
}

// one round of a row sum: this thread's four terms -> its wave's 256-element segment sum (the order of k_em_finish_b)
__device__ __forceinline__ void tw_segment(const float (&t)[4], float* seg, int s0, int nseg) {
    const float s01 = t[0] + t[1], s23 = t[2] + t[3];
    TreePath path;
    const float sum = wave_upsweep(s01 + s23, path);
    const int sg = (s0 >> 8) + ((int)threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && sg < nseg) seg[sg] = sum;
}

__device__ __forceinline__ int clamp_index(int i, int last) { return i < 0 ? 0 : (i > last ? last : i); }

__global__ void __launch_bounds__(kBlock) k_tw_gather_b(const float* __restrict__ X, const float* __restrict__ lp,
                                                        const int32_t* __restrict__ A, int n, int64_t D,
                                                        float* __restrict__ Xp, float* __restrict__ lpg) {
    const int64_t row = blockIdx.x;
    const int64_t b = row / n;
    const int32_t s = A[row];
    const int64_t src = b * n + (s < 0 ? 0 : (s > n - 1 ? n - 1 : s));
    const float* __restrict__ x = X + src * D;
    float* __restrict__ o = Xp + row * D;
    for (int64_t e = threadIdx.x; e < D; e += kBlock) o[e] = x[e];
    if (threadIdx.x == 0 && lpg) lpg[row] = lp[src];
}

template <int NETDT>
__global__ void __launch_bounds__(kBlock) k_tw_twist_b(const TwArgs a) {
    __shared__ float seg[kMaxSeg];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n);
    const int dv = a.dv, D = a.du + dv;
    const int32_t* __restrict__ v_off = a.v_off + (a.nmasks == 1 ? 0 : (int64_t)b * dv);
    const float* __restrict__ x = a.X + row * D;
    const float* __restrict__ y = a.y + (int64_t)b * dv;
    const int nseg = (dv + 255) >> 8;
    const int nsp = next_pow2(nseg > 1 ? nseg : 1);
    const float lognorm = fbsmi_logf(6.2831855f * a.var_y);
    for (int i = threadIdx.x; i < nsp; i += kBlock) seg[i] = 0.0f;
    __syncthreads();
    for (int s0 = 0; s0 < dv; s0 += 4 * kBlock) {   // uniform trip count: every wave takes part in every round
        const int j0 = s0 + (int)threadIdx.x * 4;
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = 0.0f;
            if (j0 + k < dv) {
                const int e = clamp_index(v_off[j0 + k], D - 1);
                float rd;
                const float den = tw_den(a, x[e], net_value<NETDT>(a.net, row * D + e), rd);
                t[k] = tw_nlp(y[j0 + k], den, a.var_y, lognorm);
            }
        }
        tw_segment(t, seg, s0, nseg);
    }
    lds_upsweep(seg, nsp, nsp);
    if (threadIdx.x == 0) {
        const float lp = seg[nsp - 1];
        a.lp[row] = lp;
        if (a.lw) {
            const float s1 = a.tl_in[row] + lp;
            const float s2 = s1 - a.pl_in[row];
            a.lw[row] = s2 - a.lpg[row];
        }
    }
}

// g = (y - den) / var_y on an observed element (role o < 0, observed element ~o), 0 elsewhere
template <int NETDT>
__device__ __forceinline__ float tw_head_grad(const TwArgs& a, const float* __restrict__ y, int o, float x, float s,
                                              float& rd) {
    const float den = tw_den(a, x, s, rd);
    if (o >= 0 || a.dv < 1) return 0.0f;
    const float df = y[clamp_index(~o, a.dv - 1)] - den;
    return df / a.var_y;
}

template <int NETDT>
__global__ void __launch_bounds__(kBlock) k_tw_cotangent_b(const TwArgs a) {
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n);
    const int D = a.du + a.dv;
    const int32_t* __restrict__ role = a.role + (a.nmasks == 1 ? 0 : (int64_t)b * D);
    const float* __restrict__ x = a.X + row * D;
    const float* __restrict__ y = a.y + (int64_t)b * a.dv;
    const float csdt = a.cs * a.dt;
    for (int e = threadIdx.x; e < D; e += kBlock) {
        float rd;
        const float g = tw_head_grad<NETDT>(a, y, role[e], x[e], net_value<NETDT>(a.net, row * D + e), rd);
        a.out[row * D + e] = csdt * g;
    }
}

template <int NETDT, int OUTDT>
__global__ void __launch_bounds__(kBlock) k_tw_propose_b(const TwArgs a) {
    __shared__ float seg_t[kMaxSeg], seg_p[kMaxSeg];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n), r = (int)(row - (int64_t)b * a.n);
    const int D = a.du + a.dv;
    const int32_t* __restrict__ role = a.role + (a.nmasks == 1 ? 0 : (int64_t)b * D);
    const float* __restrict__ x = a.X + row * D;
    const float* __restrict__ vjp = a.vjp + row * D;
    const float* __restrict__ y = a.y + (int64_t)b * a.dv;
    const uint32_t k0 = a.keys[2 * b], k1 = a.keys[2 * b + 1];
    const uint64_t ntot = (uint64_t)a.n * (uint64_t)D;
    const int nseg = (D + 255) >> 8;
    const int nsp = next_pow2(nseg);
    const float c1 = a.cx * a.dt;
    const float kap = 1.0f + c1;
    const float var = a.sd * a.sd;
    const float lognorm = fbsmi_logf(6.2831855f * var);
    for (int i = threadIdx.x; i < nsp; i += kBlock) seg_t[i] = seg_p[i] = 0.0f;
    __syncthreads();
    for (int s0 = 0; s0 < D; s0 += 4 * kBlock) {   // uniform trip count: every wave takes part in every round
        const int e0 = s0 + (int)threadIdx.x * 4;
        float tt[4], tp[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tt[k] = tp[k] = 0.0f;
            const int e = e0 + k;
            if (e < D) {
                const float xv = x[e];
                float rd;
                const float g = tw_head_grad<NETDT>(a, y, role[e], xv, net_value<NETDT>(a.net, row * D + e), rd);
                const float hg = kap * g;
                const float grad = hg + vjp[e];
                const float cg = a.cs * grad;
                const float cd = rd + cg;
                const float pm = cd * a.dt;
                const float m = xv + pm;
                const float z = normal_from_bits(random_bits_at(k0, k1, ntot, (uint64_t)r * D + e));
                const float nz = a.sd * z;
                const float xn = m + nz;
                const float pt = rd * a.dt;
                const float mt = xv + pt;
                a.out[row * D + e] = xn;
                if (a.out2) {
                    if (OUTDT == 0) ((float*)a.out2)[row * D + e] = xn;
                    else ((unsigned short*)a.out2)[row * D + e] = f32_to_bf16_bits(xn);
                }
                tt[k] = tw_nlp(xn, mt, var, lognorm);
                tp[k] = tw_nlp(xn, m, var, lognorm);
            }
        }
        tw_segment(tt, seg_t, s0, nseg);
        tw_segment(tp, seg_p, s0, nseg);
    }
    lds_upsweep(seg_t, nsp, nsp);
    lds_upsweep(seg_p, nsp, nsp);
    if (threadIdx.x == 0) {
        a.tl[row] = seg_t[nsp - 1];
        a.pl[row] = seg_p[nsp - 1];
    }
}

// row b of out (B) = fbsmi_categorical(keys[b], w[b]): the CDF tree of k_resample_b, one search by the first thread
__global__ void __launch_bounds__(kMaxRows) k_categorical_b(const uint32_t* __restrict__ keys, const float* __restrict__ w,
                                                            int n, int np, int32_t* __restrict__ out) {
    __shared__ float tr[kMaxRows], cdf[kMaxRows];
    const int b = blockIdx.x, e = threadIdx.x;
    tr[e] = e < n ? w[(int64_t)b * n + e] : 0.0f;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    if (e == 0) {
        const float u = uniform_at(keys[2 * b], keys[2 * b + 1], 1, 0);
        out[b] = searchsorted_left(cdf, n, bisect_levels(n), cdf[n - 1] * (1.0f - u));
    }
}

// entry b of out_i (B) = fbsmi_force_move(keys[b], w[b], k[b]) (gibbs.py:171-214): the rest weights (V_FMREST of
// fbsmi_prims.hip) scanned in LDS, both sub-keys split here, the tail of k_force_move_finish by the first thread; with
// out_alpha the tree sum of the V_FMALPHA values clipped to [0, 1].  k is clamped into [0, n) before it addresses memory,
// and so is the drawn index (which leaves [0, n) only on weights that are not numbers).
__global__ void __launch_bounds__(kMaxRows) k_force_move_b(const uint32_t* __restrict__ keys, const float* __restrict__ w,
                                                           const int32_t* __restrict__ kref, int n, int np,
                                                           int32_t* __restrict__ out_i, float* __restrict__ out_alpha) {
    __shared__ float sw[kMaxRows], tr[kMaxRows], cdf[kMaxRows];
    const int b = blockIdx.x, e = threadIdx.x;
    const int k = clamp_index(kref[b], n - 1);
    const float we = e < n ? w[(int64_t)b * n + e] : 0.0f;
    sw[e] = we;
    __syncthreads();
    const float w_k = sw[k];
    const float temp = 1.0f - w_k;
    float rest = 0.0f;
    if (e < n) {
        if (w_k < 1.0f) rest = (e == k ? 0.0f : we) / temp;
        else rest = (float)(1.0 / (double)n);
    }
    tr[e] = rest;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    if (e == 0) {
        const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
        uint32_t a0, a1, b0, b1;
        split_at(k0, k1, 2, 0, a0, a1);
        split_at(k0, k1, 2, 1, b0, b1);
        const float u1 = uniform_at(a0, a1, 1, 0);
        const int32_t i = clamp_index(searchsorted_left(cdf, n, bisect_levels(n), cdf[n - 1] * (1.0f - u1)), n - 1);
        const float u = uniform_at(b0, b1, 1, 0);
        const bool accept = u * (1.0f - sw[i]) < temp;
        out_i[b] = accept ? i : k;
    }
    if (out_alpha) {   // uniform over the workgroup
        float al = 0.0f;
        if (e < n) {
            al = temp * rest / (1.0f - we);
            al = (al != al) ? 0.0f : al;
        }
        tr[e] = al;   // every read of tr above is behind the barrier that follows the scan
        lds_upsweep(tr, np, np);
        if (e == 0) {
            const float root = tr[np - 1];
            out_alpha[b] = root < 0.0f ? 0.0f : (root > 1.0f ? 1.0f : root);
        }
    }
}

// row b of out (B, n) = fbsmi_randint(keys[b], n, lo, hi): k_randint of fbsmi_prims.hip with the key read per row.
// `bpr` workgroups per row.
__global__ void __launch_bounds__(kBlock) k_randint_b(const uint32_t* __restrict__ keys, uint64_t n, int bpr, int32_t lo,
                                                      int32_t hi, int32_t* __restrict__ out) {
    const int64_t b = blockIdx.x / bpr;
    const int q = (int)(blockIdx.x - b * bpr);
    const uint32_t k0 = keys[2 * b], k1 = keys[2 * b + 1];
    int32_t* __restrict__ o = out + b * (int64_t)n;
    for (uint64_t i = (uint64_t)q * kBlock + threadIdx.x; i < n; i += (uint64_t)bpr * kBlock)
        o[i] = randint_at(k0, k1, n, i, lo, hi);
}

// ensemble b = backward_scanning_pass (csmc/csmc.py:105-112) on its own arrays: normalise(log_w_T[b], log_space=False)
// with the arithmetic of k_normalise_b, the draw of k_categorical_b, then the first thread walks the trace
// Bs[k - 1] = As[k - 1][b][Bs[k]] and parks it in Bs; after a barrier all threads copy the rows path[b][k] = uss[k][b][Bs[k]].
// As (T, B, n) and uss (T + 1, B, n, du) are time-major, Bs (B, T + 1) and path (B, T + 1, du) batch-major.  Ancestors are
// clamped into [0, n) before they address memory.
__global__ void __launch_bounds__(kMaxRows) k_backscan_b(const uint32_t* __restrict__ keys, const float* __restrict__ lwT,
                                                         const int32_t* __restrict__ As, const float* __restrict__ uss,
                                                         int64_t B, int n, int np, int T, int64_t du, int32_t* Bs,
                                                         float* __restrict__ path) {
    __shared__ float tr[kMaxRows], cdf[kMaxRows];
    __shared__ float smax[kMaxRows / 64];
    const int64_t b = blockIdx.x;
    const int e = threadIdx.x;
    const float l = e < n ? lwT[b * n + e] : -__builtin_inff();
    const float lse = lds_row_lse(l, n, np, tr, smax);
    __syncthreads();   // the row's tree in tr has been read by everyone
    tr[e] = e < n ? fbsmi_expf(l - lse) : 0.0f;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    int32_t* bs = Bs + b * ((int64_t)T + 1);
    if (e == 0) {
        const float u = uniform_at(keys[2 * b], keys[2 * b + 1], 1, 0);
        int32_t a = clamp_index(searchsorted_left(cdf, n, bisect_levels(n), cdf[n - 1] * (1.0f - u)), n - 1);
        bs[T] = a;
        for (int k = T; k >= 1; --k) {
            a = clamp_index(As[((int64_t)(k - 1) * B + b) * n + a], n - 1);
            bs[k - 1] = a;
        }
    }
    __threadfence_block();
    __syncthreads();
    const int64_t total = ((int64_t)T + 1) * du;
    float* __restrict__ p = path + b * total;
    for (int64_t i = e; i < total; i += blockDim.x) {
        const int64_t k = i / du, c = i - k * du;
        p[i] = uss[((k * B + b) * n + bs[k]) * du + c];
    }
}

// ensemble b = k_affine_em_path (fbsmi_sde.hip) on its own keys (T, 2), target and start: the same expression under the
// same contraction setting.  Point k lands at out + (reverse ? T - k : k) * slot_stride + b * ens_stride.  `bpr`
// workgroups of 64 threads per ensemble stride over the coordinates.
__global__ void __launch_bounds__(64) k_affine_em_path_b(const uint32_t* __restrict__ keys, const float* __restrict__ A,
                                                         const float* __restrict__ Bt, const float* __restrict__ S,
                                                         const float* __restrict__ ddt, const float* __restrict__ target,
                                                         const float* __restrict__ x0, int T, int nsub, int64_t D,
                                                         int replace_last, int bpr, float* __restrict__ out,
                                                         int64_t slot_stride, int64_t ens_stride, int reverse) {
    const int64_t b = blockIdx.x / bpr;
    const int q = (int)(blockIdx.x - b * bpr);
    const uint64_t n = (uint64_t)nsub * (uint64_t)D;
    const uint32_t* __restrict__ kb = keys + b * 2 * (int64_t)T;
    float* __restrict__ o = out + b * ens_stride;
    for (int64_t c = (int64_t)q * 64 + threadIdx.x; c < D; c += (int64_t)bpr * 64) {
        float x = x0[b * D + c];
        const float tg = target[b * D + c];
        o[(reverse ? (int64_t)T : 0) * slot_stride + c] = x;
        for (int k = 0; k < T; ++k) {
            const uint32_t k0 = kb[2 * k], k1 = kb[2 * k + 1];
            const float h = ddt[k];
            const float sq = fbsmi_sqrtf(h);
            for (int j = 0; j < nsub; ++j) {
                const int r = k * nsub + j;
                const float xi = normal_at(k0, k1, n, (uint64_t)j * D + c);
                const float drift = A[r] * x + Bt[r] * tg;
                x = (x + drift * h) + (S[r] * sq) * xi;
            }
            o[(int64_t)(reverse ? T - 1 - k : k + 1) * slot_stride + c] = x;
        }
        if (replace_last) o[(reverse ? 0 : (int64_t)T) * slot_stride + c] = tg;
    }
}

// ------------------------------------------------------------------------------------------------
// forward noising paths of B ensembles (ScoreBridge.fwd_sampler_batched / fwd_ys_sampler_batched): the state is an image
// (B, D) in image order, its path is written ALREADY UNPACKED -- image position e with o = role[e] >= 0 is element o of the
// u output, o < 0 element ~o of the v output -- at base + slot * slot_stride + b * b_stride + element.  A NULL role table
// is the identity layout: every position goes to the u output, du = D.  `bpr` workgroups per ensemble, the threads of an
// ensemble stride over its positions (any D); a thread touches only its own position: no barrier, no LDS.
// ------------------------------------------------------------------------------------------------
struct PathOut {
    float* u;
    float* v;            // nullable: the observed half is not wanted
    int64_t u_slot, u_b, v_slot, v_b;
};

struct PathArgs {
    const int32_t* role;   // (nmasks, D), or NULL
    const float* x0s;      // (B, du)
    const float* y0s;      // (B, dv)
    const uint32_t* keys;  // (B, 2)
    int32_t du, dv, nmasks, bpr;
    PathOut out;
};

// where image position e of ensemble b lives: `part` (x0s or y0s row / u or v output), element o clamped into its part
// whatever the table holds; false when the position has no element (dv == 0 behind a bad table)
__device__ __forceinline__ bool path_element(const PathArgs& a, int b, int64_t e, bool& unobs, int& o) {
    const int r = a.role ? a.role[(a.nmasks == 1 ? 0 : (int64_t)b * (a.du + a.dv)) + e] : (int)e;
    unobs = r >= 0;
    o = unobs ? r : ~r;
    const int last = (unobs ? a.du : a.dv) - 1;
    o = o > last ? last : o;
    return o >= 0;
}

__device__ __forceinline__ float path_initial(const PathArgs& a, int b, bool unobs, int o) {
    return unobs ? a.x0s[(int64_t)b * a.du + o] : a.y0s[(int64_t)b * a.dv + o];
}

__device__ __forceinline__ void path_store(const PathOut& p, int b, bool unobs, int o, int64_t slot, float x) {
    if (unobs) p.u[slot * p.u_slot + b * p.u_b + o] = x;
    else if (p.v) p.v[slot * p.v_slot + b * p.v_b + o] = x;
}

// ensemble b = k_linear_path (fbsmi_sde.hip) on normal(keys[b], (T, D)), the same expression under the same contraction
// setting, with the draw made here: point k lands in slot T - k (reverse) or k
__global__ void __launch_bounds__(64) k_linear_path_b(const PathArgs a, const float* __restrict__ F,
                                                      const float* __restrict__ S, int T, int reverse) {
    const int b = blockIdx.x / a.bpr, q = blockIdx.x - b * a.bpr;
    const int D = a.du + a.dv;
    const uint32_t k0 = a.keys[2 * b], k1 = a.keys[2 * b + 1];
    const uint64_t ntot = (uint64_t)T * (uint64_t)D;
    for (int64_t e = q * 64 + (int)threadIdx.x; e < D; e += a.bpr * 64) {
        bool unobs;
        int o;
        if (!path_element(a, b, e, unobs, o)) continue;
        float x = path_initial(a, b, unobs, o);
        path_store(a.out, b, unobs, o, reverse ? T : 0, x);
        for (int k = 0; k < T; ++k) {
            const float xi = normal_at(k0, k1, ntot, (uint64_t)k * D + e);
            x = F[k] * x + S[k] * xi;
            path_store(a.out, b, unobs, o, reverse ? T - 1 - k : k + 1, x);
        }
    }
}

// ensemble b = one fbsmi_em_update (k_em_update, fbsmi_sde.hip) on its own image: out = (x + f * ddt) + c * xi with
// xi = element noff + e of normal(keys[b], (ntot,)); net == NULL assembles the initial state from x0s / y0s instead.  The
// state read and the network read are coalesced (position e of row b); x_out may be x.
template <int NETDT>
__global__ void __launch_bounds__(kBlock) k_em_fwd_step_b(const PathArgs a, const float* x, const void* __restrict__ net,
                                                          float ddt, float c, uint64_t ntot, uint64_t noff, float* x_out,
                                                          int64_t store_slot) {
    const int b = blockIdx.x / a.bpr, q = blockIdx.x - b * a.bpr;
    const int D = a.du + a.dv;
    uint32_t k0 = 0, k1 = 0;
    if (net) {
        k0 = a.keys[2 * b];
        k1 = a.keys[2 * b + 1];
    }
    for (int64_t e = q * kBlock + (int)threadIdx.x; e < D; e += a.bpr * kBlock) {
        bool unobs;
        int o;
        const bool has = path_element(a, b, e, unobs, o);
        const int64_t at = (int64_t)b * D + e;
        float out;
        if (net) {
            const float f = net_value<NETDT>(net, at);
            const float m = x[at] + f * ddt;
            const float nz = c * normal_at(k0, k1, ntot, noff + (uint64_t)e);
            out = m + nz;
        } else {
            out = has ? path_initial(a, b, unobs, o) : 0.0f;
        }
        x_out[at] = out;
        if (store_slot >= 0 && has) path_store(a.out, b, unobs, o, store_slot, out);
    }
}

// ------------------------------------------------------------------------------------------------
// backward simulation of B ensembles (samplers/smc_batched.py bootstrap_backward_smoother_batched, samplers/csmc/csmc.py
// backward_sampling_pass_batched): a step is k_em_translp_b, then k_backsim_pick_b
// ------------------------------------------------------------------------------------------------
struct TranslpArgs {
    const float* us;       // row (b, r) at us + b * us_ens + r * du
    const void* net;       // (B * n, D)
    const float* u;        // the target of ensemble b at u + b * u_ens
    float* lw;             // (B, n)
    const int32_t* u_off;  // (nmasks, du)
    int64_t us_ens, u_ens;
    int32_t du, D, nmasks, n;
    float cx, cs, dt, sd;
};

// row (b, r) = fbsmi_em_transition_logpdf of ensemble b alone: the lw loop of k_em_finish_b over the du unobserved elements,
// base the row's own us, target the ensemble's u.  One workgroup per row of the flat B * n axis.
template <int NETDT, int MODE>
__global__ void __launch_bounds__(kBlock) k_em_translp_b(const TranslpArgs a) {
    __shared__ float seg[kMaxSeg];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / a.n), r = (int)(row - (int64_t)b * a.n);
    const int du = a.du;
    const int32_t* __restrict__ u_off = a.u_off + (a.nmasks == 1 ? 0 : (int64_t)b * du);
    const float* __restrict__ x = a.us + (int64_t)b * a.us_ens + (int64_t)r * du;
    const float* __restrict__ u = a.u + (int64_t)b * a.u_ens;
    const int64_t net_row = row * a.D;
    const int nseg = (du + 255) >> 8;
    const int nsp = next_pow2(nseg);
    const float var = a.sd * a.sd;
    const float lognorm = fbsmi_logf(6.2831855f * var);
    for (int i = threadIdx.x; i < nsp; i += kBlock) seg[i] = 0.0f;
    __syncthreads();
    for (int s0 = 0; s0 < du; s0 += 4 * kBlock) {   // uniform trip count: every wave takes part in every round
        const int j0 = s0 + (int)threadIdx.x * 4;
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            t[k] = 0.0f;
            if (j0 + k < du) {
                const float sv = net_value<NETDT>(a.net, net_row + clamp_index(u_off[j0 + k], a.D - 1));
                const float bv = x[j0 + k];
                const float dr = reverse_drift<MODE>(a.cx, a.cs, bv, sv);
                const float m = bv + dr * a.dt;
                t[k] = tw_nlp(u[j0 + k], m, var, lognorm);
            }
        }
        tw_segment(t, seg, s0, nseg);
    }
    lds_upsweep(seg, nsp, nsp);
    if (threadIdx.x == 0) a.lw[row] = seg[nsp - 1];
}

// ensemble b: g = lw[b], with log_w g = (g - max(g)) + log_w[b] (csmc.py:206-208); w = normalise(g, log_space = 0) with the
// arithmetic of k_normalise_b; i = the draw and search of k_categorical_b on w; idx[b * idx_stride] = i and all threads copy
// the row us[b][i] to out[b].  blockDim.x = np; i is clamped into [0, n) before it addresses memory.
__global__ void __launch_bounds__(kMaxRows) k_backsim_pick_b(const uint32_t* __restrict__ keys, const float* __restrict__ lw,
                                                             const float* __restrict__ log_w, const float* __restrict__ us,
                                                             int64_t us_ens, int n, int np, int64_t du, int32_t* __restrict__ idx,
                                                             int64_t idx_stride, float* __restrict__ out, int64_t out_ens) {
    __shared__ float tr[kMaxRows], cdf[kMaxRows];
    __shared__ float smax[kMaxRows / 64];
    __shared__ int32_t s_pick;
    const int64_t b = blockIdx.x;
    const int e = threadIdx.x;
    float g = e < n ? lw[b * n + e] : -__builtin_inff();
    if (log_w) {   // uniform over the workgroup
        const float mw = wave_max(g);
        if ((e & 63) == 0) smax[e >> 6] = mw;
        __syncthreads();
        float m = -__builtin_inff();
        for (int q = 0; q < (np >> 6); ++q) m = fmaxf(m, smax[q]);
        __syncthreads();   // smax has been read by everyone: lds_row_lse writes it again
        if (e < n) {
            const float c = g - m;
            g = c + log_w[b * n + e];
        }
    }
    const float lse = lds_row_lse(g, n, np, tr, smax);
    __syncthreads();   // the row's tree in tr has been read by everyone
    tr[e] = e < n ? fbsmi_expf(g - lse) : 0.0f;
    lds_upsweep(tr, np, np);
    cdf[e] = lds_scan_at(tr, np, e);
    __syncthreads();
    if (e == 0) {
        const float u = uniform_at(keys[2 * b], keys[2 * b + 1], 1, 0);
        s_pick = clamp_index(searchsorted_left(cdf, n, bisect_levels(n), cdf[n - 1] * (1.0f - u)), n - 1);
    }
    __syncthreads();
    const int64_t i = s_pick;
    if (e == 0) idx[b * idx_stride] = (int32_t)i;
    const float* __restrict__ src = us + b * us_ens + i * du;
    float* __restrict__ o = out + b * out_ens;
    for (int64_t c = e; c < du; c += blockDim.x) o[c] = src[c];
}

#define FBSMI_NEED(cond, msg) \
    if (!(cond)) return fail(FBSMI_ERR_ARG, msg)
#define FBSMI_LAUNCH_CHECK()                                                 \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) return fail(FBSMI_ERR_HIP, hipGetErrorString(e_)); \
    } while (0)

int threads_for(int64_t n) {
    const int np = next_pow2((int)n);
    return np < 64 ? 64 : np;
}

constexpr int64_t kMaxGrid = ((int64_t)1 << 31) - 1;
constexpr int64_t kMaxDraw = ((int64_t)1 << 32) - 4;   // fbsmi_em_finish's bound on the flat draw of one ensemble

// the checks the two image entry points share; everything here reads values only
int check_em(const char* who, const fbsmi_em_mask_batch* m, int64_t B, int64_t n) {
    const std::string w(who);
    FBSMI_NEED(m && m->u_off && m->role && (m->dv == 0 || m->v_off), w + ": null mask");
    FBSMI_NEED(B >= 1 && n >= 1 && m->du >= 1 && m->dv >= 0, w + ": B, n and du must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, w + ": more than 1024 rows per ensemble");
    FBSMI_NEED(m->nmasks == 1 || m->nmasks == B, w + ": nmasks must be 1 or B");
    FBSMI_NEED(n * (int64_t)m->du <= kMaxDraw, w + ": the noise draw exceeds 2^32 - 4 elements");
    FBSMI_NEED(B * n <= kMaxGrid, w + ": too many rows for one grid");
    if (m->dv > kMaxSeg * 256) return fail(FBSMI_ERR_UNSUPPORTED, w + ": observed part too long");
    return FBSMI_OK;
}

// the checks the image twisted-SMC entry points share: the particles are whole images, so the draw and the row sums
// run over D = du + dv
int check_tw(const char* who, const fbsmi_em_mask_batch* m, int64_t B, int64_t n) {
    const std::string w(who);
    FBSMI_NEED(m && m->u_off && m->role && (m->dv == 0 || m->v_off), w + ": null mask");
    FBSMI_NEED(B >= 1 && n >= 1 && m->du >= 1 && m->dv >= 0, w + ": B, n and du must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, w + ": more than 1024 rows per ensemble");
    FBSMI_NEED(m->nmasks == 1 || m->nmasks == B, w + ": nmasks must be 1 or B");
    const int64_t D = (int64_t)m->du + m->dv;
    FBSMI_NEED(n * D <= kMaxDraw, w + ": the noise draw exceeds 2^32 - 4 elements");
    FBSMI_NEED(B * n <= kMaxGrid, w + ": too many rows for one grid");
    if (D > kMaxSeg * 256) return fail(FBSMI_ERR_UNSUPPORTED, w + ": image too long");
    return FBSMI_OK;
}

TwArgs tw_args(const fbsmi_em_mask_batch* m, const float* X, const void* net, const float* y, int64_t n, float cx, float cs,
               float dt, float var_y) {
    TwArgs a = {};
    a.X = X; a.net = net; a.y = y;
    a.v_off = m->v_off; a.role = m->role;
    a.du = m->du; a.dv = m->dv; a.nmasks = m->nmasks; a.n = (int32_t)n;
    a.cx = cx; a.cs = cs; a.dt = dt; a.var_y = var_y;
    return a;
}

// the checks the two forward-path entry points share, and their launch geometry (`block` threads, at most 64 workgroups
// per ensemble); everything here reads values only
int path_args(const char* who, const fbsmi_em_mask_batch* m, int64_t D, const float* x0s, const float* y0s,
              bool need_initial, const uint32_t* keys, bool need_keys, int64_t B, int block, float* out_u,
              int64_t u_slot_stride, int64_t u_b_stride, float* out_v, int64_t v_slot_stride, int64_t v_b_stride,
              PathArgs* a) {
    const std::string w(who);
    FBSMI_NEED(!m || (m->role && m->du >= 1 && m->dv >= 0), w + ": a mask needs its role table, du >= 1 and dv >= 0");
    FBSMI_NEED(D >= 1 && D <= kMaxGrid && (!m || (int64_t)m->du + m->dv == D),
               w + ": D must be in [1, 2^31 - 1] and equal du + dv of the mask");
    FBSMI_NEED(B >= 1 && B <= kMaxGrid, w + ": B must be in [1, 2^31 - 1]");
    FBSMI_NEED(!m || m->nmasks == 1 || m->nmasks == B, w + ": nmasks must be 1 or B");
    const int64_t dv = m ? m->dv : 0;
    FBSMI_NEED(!need_initial || (x0s && (dv == 0 || y0s)), w + ": null x0s or y0s");
    FBSMI_NEED(!need_keys || keys, w + ": null keys");
    int64_t bpr = (D + block - 1) / block;
    if (bpr > 64) bpr = 64;
    FBSMI_NEED(B <= kMaxGrid / bpr, w + ": too many ensembles for one grid");
    *a = PathArgs{};
    a->role = m ? m->role : nullptr;
    a->x0s = x0s; a->y0s = y0s; a->keys = keys;
    a->du = (int32_t)(D - dv); a->dv = (int32_t)dv; a->nmasks = m ? m->nmasks : 1; a->bpr = (int32_t)bpr;
    a->out = PathOut{out_u, out_v, u_slot_stride, u_b_stride, v_slot_stride, v_b_stride};
    return FBSMI_OK;
}

}  // namespace

}  // namespace fbsmi

using namespace fbsmi;

extern "C" {

int fbsmi_normalise_batched(const float* lw, int64_t B, int64_t n, int log_space, float* out, float* out_lse,
                            void* stream) {
    FBSMI_NEED(lw && out, "normalise_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && B <= kMaxGrid, "normalise_batched: B and n must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "normalise_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_normalise_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(lw, (int)n, np, log_space, out, out_lse);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_cond_killing_batched(const uint32_t* keys, const float* w, const int32_t* i, const int32_t* j, int64_t B,
                               int64_t n, int32_t* idx, void* stream) {
    FBSMI_NEED(keys && w && i && j && idx, "cond_killing_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && B <= kMaxGrid, "cond_killing_batched: B and n must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "cond_killing_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_cond_killing_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, w, i, j, (int)n, np, idx);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_concat_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const float* v_prev,
                            int64_t B, int64_t n, int out_dtype, void* img, void* stream) {
    const int rc = check_em("em_concat_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED(us && img && (mask->dv == 0 || v_prev), "em_concat_batched: null pointer");
    FBSMI_NEED(out_dtype == 0 || out_dtype == 1, "em_concat_batched: out_dtype must be 0 or 1");
    BatchArgs a = {};
    a.us = us; a.A = A; a.v_prev = v_prev; a.role = mask->role; a.img = img;
    a.du = mask->du; a.dv = mask->dv; a.nmasks = mask->nmasks; a.n = (int32_t)n;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == 0) k_em_concat_b<0><<<grid, kBlock, 0, st>>>(a);
    else k_em_concat_b<1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_finish_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const void* net,
                            int net_dtype, int mode, float cx, float cs, float dt, float sd, const float* v,
                            const float* v_prev, const uint32_t* keys, int64_t B, int64_t n, const int32_t* pin_row,
                            const float* pin_value, float* us_new, float* lw, void* stream) {
    const int rc = check_em("em_finish_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED(net && (us_new || lw), "em_finish_batched: null network output, or neither us_new nor lw asked for");
    FBSMI_NEED((net_dtype == 0 || net_dtype == 1) && (mode == 0 || mode == 1), "em_finish_batched: bad net_dtype or mode");
    FBSMI_NEED(!us_new || (us && keys && us_new != us), "em_finish_batched: the proposal needs us and keys, and us_new must not alias us");
    FBSMI_NEED(!lw || mask->dv == 0 || (v && v_prev), "em_finish_batched: the weights need v and v_prev");
    FBSMI_NEED(!pin_row || pin_value, "em_finish_batched: pin_row without pin_value");
    BatchArgs a = {};
    a.us = us; a.A = A; a.net = net; a.v = v; a.v_prev = v_prev; a.keys = keys;
    a.pin_row = us_new ? pin_row : nullptr; a.pin_value = pin_value; a.us_new = us_new; a.lw = lw;
    a.u_off = mask->u_off; a.v_off = mask->v_off;
    a.du = mask->du; a.dv = mask->dv; a.nmasks = mask->nmasks; a.n = (int32_t)n;
    a.cx = cx; a.cs = cs; a.dt = dt; a.sd = sd;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0 && mode == 0) k_em_finish_b<0, 0><<<grid, kBlock, 0, st>>>(a);
    else if (net_dtype == 0) k_em_finish_b<0, 1><<<grid, kBlock, 0, st>>>(a);
    else if (mode == 0) k_em_finish_b<1, 0><<<grid, kBlock, 0, st>>>(a);
    else k_em_finish_b<1, 1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_resample_batched(int kind, const uint32_t* keys, const float* w, int64_t B, int64_t n, int32_t* idx,
                           void* stream) {
    FBSMI_NEED(kind >= 0 && kind <= 3, "resample_batched: kind must be 0..3");
    FBSMI_NEED(keys && w && idx, "resample_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && B <= kMaxGrid, "resample_batched: B and n must be at least 1");
    if (kind > 1) return fail(FBSMI_ERR_UNSUPPORTED, "resample_batched: stratified (0) and systematic (1) only");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "resample_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_resample_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, w, (int)n, np, kind == 1, idx);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_propose_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const void* net,
                             int net_dtype, int mode, float cx, float cs, float dt, float sd, const uint32_t* keys,
                             int64_t B, int64_t n, float* us_new, void* stream) {
    FBSMI_NEED(us && A && net && keys && us_new, "em_propose_batched: null pointer");
    const int rc = check_em("em_propose_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED((net_dtype == 0 || net_dtype == 1) && (mode == 0 || mode == 1), "em_propose_batched: bad net_dtype or mode");
    FBSMI_NEED(us_new != us, "em_propose_batched: us_new must not alias us");
    BatchArgs a = {};
    a.us = us; a.A = A; a.net = net; a.keys = keys; a.us_new = us_new;
    a.u_off = mask->u_off; a.v_off = mask->v_off;
    a.du = mask->du; a.dv = mask->dv; a.nmasks = mask->nmasks; a.n = (int32_t)n;
    a.cx = cx; a.cs = cs; a.dt = dt; a.sd = sd;
    a.net_by_A = 1;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0 && mode == 0) k_em_finish_b<0, 0><<<grid, kBlock, 0, st>>>(a);
    else if (net_dtype == 0) k_em_finish_b<0, 1><<<grid, kBlock, 0, st>>>(a);
    else if (mode == 0) k_em_finish_b<1, 0><<<grid, kBlock, 0, st>>>(a);
    else k_em_finish_b<1, 1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_csgm_step_batched(const fbsmi_em_mask_batch* mask, const float* u, const void* net, int net_dtype, float cx,
                               float cs, float dt, float c, const uint32_t* scan_keys, int64_t noise_total,
                               int64_t noise_offset, const float* y0, float F, float sq, const uint32_t* est_keys,
                               int out_dtype, void* img, int64_t B, float* u_new, void* stream) {
    FBSMI_NEED(mask && mask->u_off && mask->role && (mask->dv == 0 || mask->v_off), "em_csgm_step_batched: null mask");
    FBSMI_NEED(mask->du >= 1 && mask->dv >= 0 && (int64_t)mask->du + mask->dv <= kMaxGrid,
               "em_csgm_step_batched: du must be at least 1, dv at least 0 and du + dv below 2^31");
    FBSMI_NEED(u && (mask->dv == 0 || y0) && scan_keys && est_keys, "em_csgm_step_batched: null u, y0 or keys");
    FBSMI_NEED(net || img, "em_csgm_step_batched: neither the update (net) nor the network input (img) asked for");
    FBSMI_NEED(!net || u_new, "em_csgm_step_batched: net without u_new");
    FBSMI_NEED(B >= 1 && B <= kMaxGrid, "em_csgm_step_batched: B must be in [1, 2^31 - 1]");
    FBSMI_NEED(mask->nmasks == 1 || mask->nmasks == B, "em_csgm_step_batched: nmasks must be 1 or B");
    FBSMI_NEED((net_dtype == 0 || net_dtype == 1) && (out_dtype == 0 || out_dtype == 1),
               "em_csgm_step_batched: net_dtype and out_dtype must be 0 or 1");
    FBSMI_NEED(noise_offset >= 0 && noise_total >= 0 && noise_offset <= noise_total - mask->du,
               "em_csgm_step_batched: the step's noise [noise_offset, noise_offset + du) must lie inside noise_total");
    FBSMI_NEED(noise_total <= kMaxDraw, "em_csgm_step_batched: the noise draw exceeds 2^32 - 4 elements");
    BatchArgs a = {};
    a.us = u; a.net = net; a.v_prev = y0; a.keys = scan_keys; a.us_new = net ? u_new : nullptr;
    a.role = mask->role; a.img = img;
    a.du = mask->du; a.dv = mask->dv; a.nmasks = mask->nmasks; a.n = 1;
    a.cx = cx; a.cs = cs; a.dt = dt; a.sd = c;
    const dim3 grid((unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    const uint64_t nt = (uint64_t)noise_total, no = (uint64_t)noise_offset;
    if (net_dtype == 0 && out_dtype == 0) k_em_csgm_step_b<0, 0><<<grid, kBlock, 0, st>>>(a, est_keys, F, sq, nt, no);
    else if (net_dtype == 0) k_em_csgm_step_b<0, 1><<<grid, kBlock, 0, st>>>(a, est_keys, F, sq, nt, no);
    else if (out_dtype == 0) k_em_csgm_step_b<1, 0><<<grid, kBlock, 0, st>>>(a, est_keys, F, sq, nt, no);
    else k_em_csgm_step_b<1, 1><<<grid, kBlock, 0, st>>>(a, est_keys, F, sq, nt, no);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_normal_batched(const uint32_t* keys, int64_t B, int64_t n, float* out, void* stream) {
    FBSMI_NEED(B >= 1 && n >= 0, "normal_batched: B must be at least 1 and n at least 0");
    FBSMI_NEED(keys && (n == 0 || out), "normal_batched: null pointer");
    FBSMI_NEED(n <= kMaxDraw, "normal_batched: a row exceeds 2^32 - 4 elements");
    if (n == 0) return FBSMI_OK;
    int64_t bpr = ((n + 1) / 2 + kBlock - 1) / kBlock;   // a thread per pair of elements, at most 64 workgroups per row
    if (bpr > 64) bpr = 64;
    FBSMI_NEED(B <= kMaxGrid / bpr, "normal_batched: too many rows for one grid");
    k_normal_b<<<(unsigned)(B * bpr), kBlock, 0, (hipStream_t)stream>>>(keys, (uint64_t)n, (int)bpr, out);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_tw_img_gather_batched(const float* X, const float* lp, const int32_t* A, int64_t B, int64_t n, int64_t D,
                                float* Xp, float* lp_prev_g, void* stream) {
    FBSMI_NEED(X && A && Xp && (!lp_prev_g || lp), "tw_img_gather_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && D >= 1, "tw_img_gather_batched: B, n and D must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "tw_img_gather_batched: more than 1024 rows per ensemble");
    FBSMI_NEED(D <= kMaxDraw && n * D <= kMaxDraw, "tw_img_gather_batched: an ensemble exceeds 2^32 - 4 elements");
    FBSMI_NEED(B * n <= kMaxGrid, "tw_img_gather_batched: too many rows for one grid");
    FBSMI_NEED(Xp != X, "tw_img_gather_batched: Xp must not alias X");
    k_tw_gather_b<<<(unsigned)(B * n), kBlock, 0, (hipStream_t)stream>>>(X, lp, A, (int)n, D, Xp, lp_prev_g);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_tw_img_twist_batched(const fbsmi_em_mask_batch* mask, const float* X, const void* net, int net_dtype, float cx,
                               float cs, float dt, float var_y, const float* y, const float* tl, const float* pl,
                               const float* lp_prev_g, int64_t B, int64_t n, float* lp, float* lw, void* stream) {
    const int rc = check_tw("tw_img_twist_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED(X && net && lp && (mask->dv == 0 || y), "tw_img_twist_batched: null pointer");
    FBSMI_NEED(net_dtype == 0 || net_dtype == 1, "tw_img_twist_batched: net_dtype must be 0 or 1");
    FBSMI_NEED(!lw || (tl && pl && lp_prev_g), "tw_img_twist_batched: the weights need tl, pl and lp_prev_g");
    TwArgs a = tw_args(mask, X, net, y, n, cx, cs, dt, var_y);
    a.tl_in = tl; a.pl_in = pl; a.lpg = lp_prev_g; a.lp = lp; a.lw = lw;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0) k_tw_twist_b<0><<<grid, kBlock, 0, st>>>(a);
    else k_tw_twist_b<1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_tw_img_cotangent_batched(const fbsmi_em_mask_batch* mask, const float* X, const void* net, int net_dtype,
                                   float cx, float cs, float dt, float var_y, const float* y, int64_t B, int64_t n,
                                   float* ct, void* stream) {
    const int rc = check_tw("tw_img_cotangent_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED(X && net && ct && (mask->dv == 0 || y), "tw_img_cotangent_batched: null pointer");
    FBSMI_NEED(net_dtype == 0 || net_dtype == 1, "tw_img_cotangent_batched: net_dtype must be 0 or 1");
    TwArgs a = tw_args(mask, X, net, y, n, cx, cs, dt, var_y);
    a.out = ct;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0) k_tw_cotangent_b<0><<<grid, kBlock, 0, st>>>(a);
    else k_tw_cotangent_b<1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_tw_img_propose_batched(const fbsmi_em_mask_batch* mask, const float* Xp, const void* net, int net_dtype,
                                 const float* vjp, float cx, float cs, float dt, float sd, float var_y, const float* y,
                                 const uint32_t* keys, int64_t B, int64_t n, float* X_new, float* tl, float* pl,
                                 int out_dtype, void* X_new_net, void* stream) {
    const int rc = check_tw("tw_img_propose_batched", mask, B, n);
    if (rc) return rc;
    FBSMI_NEED(Xp && net && vjp && keys && X_new && tl && pl && (mask->dv == 0 || y),
               "tw_img_propose_batched: null pointer");
    FBSMI_NEED((net_dtype == 0 || net_dtype == 1) && (out_dtype == 0 || out_dtype == 1),
               "tw_img_propose_batched: net_dtype and out_dtype must be 0 or 1");
    FBSMI_NEED(X_new != Xp && X_new_net != (const void*)Xp, "tw_img_propose_batched: X_new must not alias Xp");
    TwArgs a = tw_args(mask, Xp, net, y, n, cx, cs, dt, var_y);
    a.vjp = vjp; a.keys = keys; a.sd = sd; a.out = X_new; a.out2 = X_new_net; a.tl = tl; a.pl = pl;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0 && out_dtype == 0) k_tw_propose_b<0, 0><<<grid, kBlock, 0, st>>>(a);
    else if (net_dtype == 0) k_tw_propose_b<0, 1><<<grid, kBlock, 0, st>>>(a);
    else if (out_dtype == 0) k_tw_propose_b<1, 0><<<grid, kBlock, 0, st>>>(a);
    else k_tw_propose_b<1, 1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_categorical_batched(const uint32_t* keys, const float* w, int64_t B, int64_t n, int32_t* out, void* stream) {
    FBSMI_NEED(keys && w && out, "categorical_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && B <= kMaxGrid, "categorical_batched: B and n must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "categorical_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_categorical_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, w, (int)n, np, out);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_linear_path_batched(const fbsmi_em_mask_batch* mask, int64_t D, const float* F, const float* S, const float* x0s,
                              const float* y0s, const uint32_t* keys, int64_t B, int32_t T, int reverse, float* out_u,
                              int64_t u_slot_stride, int64_t u_b_stride, float* out_v, int64_t v_slot_stride,
                              int64_t v_b_stride, void* stream) {
    FBSMI_NEED(T >= 0 && (T == 0 || (F && S)) && out_u, "linear_path_batched: T < 0, or null F, S or out_u");
    PathArgs a;
    const int rc = path_args("linear_path_batched", mask, D, x0s, y0s, true, keys, true, B, 64, out_u, u_slot_stride,
                             u_b_stride, out_v, v_slot_stride, v_b_stride, &a);
    if (rc) return rc;
    FBSMI_NEED((int64_t)T * D <= kMaxDraw, "linear_path_batched: the noise draw exceeds 2^32 - 4 elements");
    k_linear_path_b<<<(unsigned)(B * a.bpr), 64, 0, (hipStream_t)stream>>>(a, F, S, (int)T, reverse != 0);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_fwd_step_batched(const fbsmi_em_mask_batch* mask, int64_t D, const float* x0s, const float* y0s, const float* x,
                              const void* net, int net_dtype, float ddt, float c, const uint32_t* keys, int64_t noise_total,
                              int64_t noise_offset, int64_t B, float* x_out, int64_t store_slot, float* out_u,
                              int64_t u_slot_stride, int64_t u_b_stride, float* out_v, int64_t v_slot_stride,
                              int64_t v_b_stride, void* stream) {
    FBSMI_NEED((!net || x) && (store_slot < 0 || out_u), "em_fwd_step_batched: net without x, or store_slot without out_u");
    PathArgs a;
    const int rc = path_args("em_fwd_step_batched", mask, D, x0s, y0s, net == nullptr, keys, net != nullptr, B, kBlock,
                             out_u, u_slot_stride, u_b_stride, out_v, v_slot_stride, v_b_stride, &a);
    if (rc) return rc;
    FBSMI_NEED(net_dtype == 0 || net_dtype == 1, "em_fwd_step_batched: net_dtype must be 0 or 1");
    if (net) {
        FBSMI_NEED(noise_offset >= 0 && noise_total >= 0 && noise_offset <= noise_total - D,
                   "em_fwd_step_batched: the step's noise [noise_offset, noise_offset + D) must lie inside noise_total");
        FBSMI_NEED(noise_total <= kMaxDraw, "em_fwd_step_batched: the noise draw exceeds 2^32 - 4 elements");
    }
    FBSMI_NEED(x_out, "em_fwd_step_batched: null x_out");
    const dim3 grid((unsigned)(B * a.bpr));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t nt = (uint64_t)noise_total, no = (uint64_t)noise_offset;
    if (net_dtype == 0) k_em_fwd_step_b<0><<<grid, kBlock, 0, st>>>(a, x, net, ddt, c, nt, no, x_out, store_slot);
    else k_em_fwd_step_b<1><<<grid, kBlock, 0, st>>>(a, x, net, ddt, c, nt, no, x_out, store_slot);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_force_move_batched(const uint32_t* keys, const float* w, const int32_t* k, int64_t B, int64_t n, int32_t* out_i,
                             float* out_alpha, void* stream) {
    FBSMI_NEED(keys && w && k && out_i, "force_move_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && B <= kMaxGrid, "force_move_batched: B and n must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "force_move_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_force_move_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, w, k, (int)n, np, out_i, out_alpha);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_randint_batched(const uint32_t* keys, int64_t B, int64_t n, int32_t lo, int32_t hi, int32_t* out, void* stream) {
    FBSMI_NEED(B >= 1 && n >= 0, "randint_batched: B must be at least 1 and n at least 0");
    FBSMI_NEED(keys && (n == 0 || out), "randint_batched: null pointer");
    FBSMI_NEED(n <= kMaxDraw, "randint_batched: a row exceeds 2^32 - 4 elements");
    if (n == 0) return FBSMI_OK;
    int64_t bpr = (n + kBlock - 1) / kBlock;   // a thread per element, at most 64 workgroups per row
    if (bpr > 64) bpr = 64;
    FBSMI_NEED(B <= kMaxGrid / bpr, "randint_batched: too many rows for one grid");
    k_randint_b<<<(unsigned)(B * bpr), kBlock, 0, (hipStream_t)stream>>>(keys, (uint64_t)n, (int)bpr, lo, hi, out);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_backscan_batched(const uint32_t* keys, const float* log_w_T, const int32_t* As, const float* uss, int64_t B,
                           int64_t n, int32_t T, int64_t du, int32_t* Bs, float* path, void* stream) {
    FBSMI_NEED(keys && log_w_T && uss && Bs && path && T >= 0 && (T == 0 || As), "backscan_batched: null pointer or T < 0");
    FBSMI_NEED(B >= 1 && n >= 1 && du >= 1 && B <= kMaxGrid, "backscan_batched: B, n and du must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "backscan_batched: more than 1024 rows per ensemble");
    const int np = threads_for(n);
    k_backscan_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, log_w_T, As, uss, B, (int)n, np, (int)T, du, Bs, path);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_em_translp_batched(const fbsmi_em_mask_batch* mask, const float* us, int64_t us_ens_stride, const void* net,
                             int net_dtype, int mode, float cx, float cs, float dt, float sd, const float* u,
                             int64_t u_ens_stride, int64_t B, int64_t n, float* lw, void* stream) {
    FBSMI_NEED(mask && mask->u_off && us && net && u && lw, "em_translp_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && mask->du >= 1 && mask->dv >= 0, "em_translp_batched: B, n and du must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "em_translp_batched: more than 1024 rows per ensemble");
    FBSMI_NEED(mask->nmasks == 1 || mask->nmasks == B, "em_translp_batched: nmasks must be 1 or B");
    FBSMI_NEED((net_dtype == 0 || net_dtype == 1) && (mode == 0 || mode == 1), "em_translp_batched: bad net_dtype or mode");
    FBSMI_NEED(us_ens_stride >= 0 && u_ens_stride >= 0, "em_translp_batched: negative stride");
    FBSMI_NEED(B * n <= kMaxGrid, "em_translp_batched: too many rows for one grid");
    if (mask->du > kMaxSeg * 256) return fail(FBSMI_ERR_UNSUPPORTED, "em_translp_batched: unobserved part too long");
    TranslpArgs a = {};
    a.us = us; a.net = net; a.u = u; a.lw = lw; a.u_off = mask->u_off;
    a.us_ens = us_ens_stride; a.u_ens = u_ens_stride;
    a.du = mask->du; a.D = mask->du + mask->dv; a.nmasks = mask->nmasks; a.n = (int32_t)n;
    a.cx = cx; a.cs = cs; a.dt = dt; a.sd = sd;
    const dim3 grid((unsigned)(B * n));
    hipStream_t st = (hipStream_t)stream;
    if (net_dtype == 0 && mode == 0) k_em_translp_b<0, 0><<<grid, kBlock, 0, st>>>(a);
    else if (net_dtype == 0) k_em_translp_b<0, 1><<<grid, kBlock, 0, st>>>(a);
    else if (mode == 0) k_em_translp_b<1, 0><<<grid, kBlock, 0, st>>>(a);
    else k_em_translp_b<1, 1><<<grid, kBlock, 0, st>>>(a);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_backsim_pick_batched(const uint32_t* keys, const float* lw, const float* log_w, const float* us,
                               int64_t us_ens_stride, int64_t B, int64_t n, int64_t du, int32_t* idx, int64_t idx_stride,
                               float* out, int64_t out_ens_stride, void* stream) {
    FBSMI_NEED(keys && lw && us && idx && out, "backsim_pick_batched: null pointer");
    FBSMI_NEED(B >= 1 && n >= 1 && du >= 1 && B <= kMaxGrid, "backsim_pick_batched: B, n and du must be at least 1");
    if (n > kMaxRows) return fail(FBSMI_ERR_UNSUPPORTED, "backsim_pick_batched: more than 1024 rows per ensemble");
    FBSMI_NEED(us_ens_stride >= 0 && idx_stride >= 0 && out_ens_stride >= 0, "backsim_pick_batched: negative stride");
    const int np = threads_for(n);
    k_backsim_pick_b<<<(unsigned)B, np, 0, (hipStream_t)stream>>>(keys, lw, log_w, us, us_ens_stride, (int)n, np, du, idx,
                                                                  idx_stride, out, out_ens_stride);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_affine_em_path_batched(const uint32_t* keys, const float* A, const float* Bt, const float* S, const float* ddt,
                                 const float* target, const float* x0, int32_t T, int32_t nsub, int64_t D, int replace_last,
                                 int64_t B, float* out, int64_t slot_stride, int64_t ens_stride, int reverse, void* stream) {
    FBSMI_NEED(target && x0 && out && T >= 0 && nsub >= 1 && D >= 1 && (T == 0 || (keys && A && Bt && S && ddt)),
               "affine_em_path_batched: null pointer, T < 0, nsub < 1 or D < 1");
    FBSMI_NEED(B >= 1 && B <= kMaxGrid, "affine_em_path_batched: B must be in [1, 2^31 - 1]");
    FBSMI_NEED((int64_t)nsub * D <= kMaxDraw && (int64_t)T * nsub <= kMaxGrid,
               "affine_em_path_batched: an interval's noise draw exceeds 2^32 - 4 elements, or T * nsub exceeds 2^31 - 1");
    FBSMI_NEED(slot_stride >= 0 && ens_stride >= 0, "affine_em_path_batched: negative stride");
    int64_t bpr = (D + 63) / 64;   // a thread per coordinate, at most 64 workgroups per ensemble
    if (bpr > 64) bpr = 64;
    FBSMI_NEED(B <= kMaxGrid / bpr, "affine_em_path_batched: too many ensembles for one grid");
    k_affine_em_path_b<<<(unsigned)(B * bpr), 64, 0, (hipStream_t)stream>>>(keys, A, Bt, S, ddt, target, x0, (int)T, (int)nsub, D,
                                                                            replace_last != 0, (int)bpr, out, slot_stride,
                                                                            ens_stride, reverse != 0);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

}  // extern "C"
