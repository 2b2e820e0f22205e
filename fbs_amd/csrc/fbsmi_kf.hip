// fbsmi_kf.hip -- batched, device-resident Kalman-filter conditional sampler for the analytic linear-Gaussian model
// (include/fbsmi.h, fbsmi_kf_*): the exact filtering law p(u_T | v_0..v_T) and marginal likelihood of the discretised
// model that bootstrap_filter targets, a draw from it, for B independent samples per call.
//
// The covariance recursion does not depend on the data and is done once on the host (fbs_amd/lg_kalman.py); what is left
// per sample and step is the mean recursion in innovation form -- two dependent groups of matrix-vector products -- and a
// quadratic form.  A call is two plain launches on the caller's stream:
//   k_kf_front  one workgroup per sample: keys, the forward observation path written reversed into the handle's vs
//               (sample mode), the float64 conditional mean m_0 of ref_sampler.
//   k_kf        a workgroup (4 waves) owns 16 samples for all T steps.  The samples are the 16 columns of
//               v_mfma_f32_16x16x4_f32 (an ascending fmaf chain, bit for bit: tools/mfmatest.hip), the table rows its
//               rows; the row tiles of the u rows (Pm, AK, L) and of the v rows (H, W) are dealt round-robin to the waves
//               (tile w, w + 4 on wave w).
//   * Tables.  fbsmi_kf_create repacks H, Pm, AK, W and the transposed Lt once into the lane order of the A operand,
//     rows zero-padded to 16-row tiles and the u and v column blocks each to 16-column groups: one coalesced 16-byte
//     load per lane is the operand of four consecutive MFMAs, the padding contributes exactly +0 and no address needs a
//     clamp.  Four tables of one step do not fit the register file at d = 128 beside their successors, so the operands are
//     fetched in a rolling window kKfAhead column groups ahead of the chain that consumes them, and the first kKfAhead
//     groups of the next phase are in flight under the current one.
//   * State.  z = (m, vs[k]) sits in LDS in the plane layout of fbsmi_lg.hip's wide_pos (lane l reads its four-MFMA
//     operand as one ds_read_b128 at l * S + 4 q), ping-ponged; the innovation r and the whitened innovation qv have a
//     tile each.  Two barriers per step: behind r, and behind (m', qv).
//   * Pm z does not depend on r and runs in the same loop as H z; only the AK r and W r tails are behind the innovation.
//   * Sum of squares.  sum_i qv_i^2 is the diagonal of the 16 x 16 Gram matrix of the qv tile, one MFMA chain on wave 0
//     under the next step's first phase: acc = 0, acc = fmaf(qv_i, qv_i, acc), i ascending.
// LDS: 2 z tiles of 64 * 68 floats, r and qv tiles of 64 * 36 floats, 53 248 bytes, static.
//
// A model whose forward process is Euler-Maruyama (the Gaussian Schrodinger bridge; fbsmi_kf_set_em_forward) takes
// k_kf_front_em (fbsmi_kf_em.hip) for k_kf_front<true>: x0 and the joint path of fbsmi_em_path.h, its y half written
// reversed into vs.  That kernel is a translation unit of its own so that the kernels here compile to the code they had.
//
// fbsmi_kfs_* (the smoother and path sampler, further down) is built on the same pieces: a storing instantiation of k_kf
// that writes every m_k and r_k as it goes, and k_kfs_back, the backward recursion over them in the same layout.
#include <new>
#include <vector>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"
#include "fbsmi_kf_em.h"

using namespace fbsmi;

namespace {

constexpr int kKfTile = 16;          // samples per workgroup
constexpr int kKfMaxD = 128;         // du, dv
constexpr int kKfS1 = 36;            // kf_plane_row(128)
constexpr int kKfSz = 68;            // kf_plane_row(256)
constexpr int kKfChunk = 8;          // steps of the forward path whose draws are issued together
constexpr int kKfAhead = 2;          // column groups a table operand is asked for ahead of the chain that consumes it
typedef float mfma_f4 __attribute__((ext_vector_type(4)));

struct KfDev {
    int du, dv, T, NQu, NQv, Sz, Sv, Su;
    const float4 *Hp, *Pp, *AKp, *Wp, *Lp;   // [T][NQv][NQz][64] [T][NQu][NQz][64] [T][NQu][NQv][64] [T][NQv][NQv][64] [NQu][NQu][64]
    const float *ep, *cp, *lconst;           // [T][16 NQv] [T][16 NQu] [T]
    const float* m0;                         // [B][du]
};

// the last argument of k_kf: nothing (fbsmi_kf_*), or where every m_k and r_k goes (fbsmi_kfs_*)
struct KfNoStore {
    static constexpr bool on = false;
};
struct KfStore {
    static constexpr bool on = true;
    float *ms, *rs;                          // [B][T+1][du] [B][T][dv]
};

// what the front launch reads and writes
struct KfFront {
    int du, dv, T;
    const float *F, *sqQ;                    // [T]
    const double *m_u, *m_v, *gain;          // (du) (dv) (du, dv)
    float* vs;                               // [B][T+1][dv]
    float* m0;                               // [B][du]
};

// A row index the compiler takes as new at every use: a store predicate formed from it is a compare where it is used,
// not a lane mask held in two scalar registers across the step loop (eight of them do not fit beside the loop's state).
__device__ __forceinline__ int kf_fresh(int r) {
    asm volatile("" : "+v"(r));
    return r;
}

// wide_pos of fbsmi_lg.hip for a 16-row tile: element (sample i, column c), S floats per plane row
__device__ __forceinline__ int kf_pos(int i, int c, int S) { return ((c & 3) * kKfTile + i) * S + (c >> 2); }
inline int kf_plane_row(int Kp) { return ((Kp / 4) & 4) ? Kp / 4 : Kp / 4 + 4; }

// One matrix family to the A-operand lane order.  Source: ntab tables of R rows, `ld` floats apart, whose columns
// [0, C1) go to the padded columns [0, 16 Q1) and [C1, C1 + C2) to those from 16 Q1 on; transpose: element (r, c) is
// src[c * ld + r].  One thread per float of the packed tables.
struct KfPack {
    const float* src;
    float* dst;
    int ntab, R, C1, C2, Q1, NQr, NQc, ld, transpose;
    size_t stride;   // floats between tables of the source
};

__global__ void __launch_bounds__(kBlock) k_kf_pack(KfPack j) {
    const size_t per = (size_t)j.NQr * j.NQc * 256, total = (size_t)j.ntab * per;
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int t = (int)(e / per);
    const int w = (int)(e - (size_t)t * per);
    const int mm = w & 3, l = (w >> 2) & 63, q = (w >> 8) % j.NQc, rt = (w >> 8) / j.NQc;
    const int r = 16 * rt + (l & 15), cp = 16 * q + 4 * mm + (l >> 4);
    int c = -1;
    if (cp < 16 * j.Q1) {
        if (cp < j.C1) c = cp;
    } else if (cp - 16 * j.Q1 < j.C2) {
        c = j.C1 + cp - 16 * j.Q1;
    }
    float v = 0.0f;
    if (r < j.R && c >= 0) v = j.src[(size_t)t * j.stride + (j.transpose ? (size_t)c * j.ld + r : (size_t)r * j.ld + c)];
    j.dst[e] = v;
}

// rows of n floats to rows of Kp floats, zero padded
__global__ void __launch_bounds__(kBlock) k_kf_pad(const float* src, float* dst, int T, int n, int Kp) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= (size_t)T * Kp) return;
    const int t = (int)(e / Kp), r = (int)(e - (size_t)t * Kp);
    dst[e] = r < n ? src[(size_t)t * n + r] : 0.0f;
}

// DRAW: key_fwd = split(key, 3)[0], the forward observation path written reversed into the handle's vs (the front of
// fbsmi_lg_fsamp: thread j < dv owns coordinate j and draws normal(key_fwd, (T, dv))[k][j] where it consumes it, the draws
// of kKfChunk steps issued together ahead of the chunk's dependent chain).  Both modes: the float64 conditional mean of
// ref_sampler from vs[b][0].  Threads from dv on run coordinate dv - 1 again and store nothing.
template <bool DRAW>
__global__ void __launch_bounds__(kKfMaxD) k_kf_front(KfFront d, const uint32_t* __restrict__ keys, const float* __restrict__ y0,
                                                      const float* __restrict__ vs_in) {
    const int b = blockIdx.x;
    __shared__ uint32_t sk[2];
    __shared__ float syT[kKfMaxD];
    const int T = d.T, dv = d.dv;
    const bool live = (int)threadIdx.x < dv;
    const int j = live ? (int)threadIdx.x : dv - 1;
    if (DRAW) {
        if (threadIdx.x == 0) split_at(keys[2 * b], keys[2 * b + 1], 3, 0, sk[0], sk[1]);
        __syncthreads();
        const uint32_t s0 = sk[0], s1 = sk[1];
        const uint64_t n = (uint64_t)T * dv;
        float* vs = d.vs + (size_t)b * ((size_t)T + 1) * dv;
        float r = y0[j];
        if (live) vs[(size_t)T * dv + j] = r;                                // vs[k] = r[T - k]
        for (int k0 = 0; k0 < T; k0 += kKfChunk) {
            float f[kKfChunk], sq[kKfChunk], z[kKfChunk];
#pragma unroll
            for (int i = 0; i < kKfChunk; ++i) {
                const int k = k0 + i < T ? k0 + i : T - 1;
                f[i] = d.F[k];
                sq[i] = d.sqQ[k];
                z[i] = normal_at(s0, s1, n, (uint64_t)k * dv + j);
            }
#pragma unroll
            for (int i = 0; i < kKfChunk; ++i) {
                if (k0 + i < T) {
                    r = f[i] * r + sq[i] * z[i];
                    if (live) vs[(size_t)(T - 1 - k0 - i) * dv + j] = r;
                }
            }
        }
        if (live) syT[j] = r;                                                // yT = vs[0]
    } else {
        if (live) syT[j] = vs_in[(size_t)b * ((size_t)T + 1) * dv + j];
    }
    __syncthreads();
    for (int u = threadIdx.x; u < d.du; u += blockDim.x) {
        double s = 0.0;
        for (int cc = 0; cc < dv; ++cc) s = s + d.gain[(size_t)u * dv + cc] * ((double)syT[cc] - d.m_v[cc]);
        d.m0[(size_t)b * d.du + u] = (float)(d.m_u[u] + s);
    }
}

#define KF_MFMA4(acc, a, x)                                                      \
    do {                                                                         \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).x, (x).x, acc, 0, 0, 0);  \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).y, (x).y, acc, 0, 0, 0);  \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).z, (x).z, acc, 0, 0, 0);  \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).w, (x).w, acc, 0, 0, 0);  \
    } while (0)

// The mean recursion, the log-likelihood and (DRAW) the draw for the 16 samples of a workgroup.  vs: the handle's buffer
// (sample mode) or the caller's paths (filter mode), (B, T+1, dv); m0 is the front's.  STORE (fbsmi_kfs_*): every m_k
// and r_k is written to st.ms and st.rs as the step produces it; the arithmetic is the same, and the instantiations
// without stores keep the arguments they had and, with them, their code.
template <bool DRAW, class Store = KfNoStore>
__global__ void __launch_bounds__(kBlock) k_kf(KfDev d, const float* __restrict__ vs, const uint32_t* __restrict__ keys,
                                               float* __restrict__ samples, float* __restrict__ means,
                                               float* __restrict__ loglik, int B, Store st = Store()) {
    constexpr bool STORE = Store::on;
    __shared__ __attribute__((aligned(16))) float zs[2][4 * kKfTile * kKfSz];
    __shared__ __attribute__((aligned(16))) float rs[4 * kKfTile * kKfS1];
    __shared__ __attribute__((aligned(16))) float qs[4 * kKfTile * kKfS1];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int du = d.du, dv = d.dv, T = d.T, NQu = d.NQu, NQv = d.NQv, NQz = NQu + NQv;
    const int Sz = d.Sz, Sv = d.Sv, Ku = 16 * NQu, Kv = 16 * NQv;
    const int smp = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x * kKfTile + smp;
    const bool live = b < B;
    const int bc = live ? b : B - 1;   // the slots past the batch repeat its last sample and store nothing
    const float* vsb = vs + (size_t)bc * ((size_t)T + 1) * dv;   // this lane's sample, advanced a step per step
    // the loader's view of the tile: sample t / 16, columns t % 16 + 16 j (16 consecutive floats per 16 lanes)
    const int ls = t >> 4, lc = t & 15;
    const int lb = blockIdx.x * kKfTile + ls < B ? blockIdx.x * kKfTile + ls : B - 1;
    const float* vsl = vs + (size_t)lb * ((size_t)T + 1) * dv;   // the loader's sample, likewise
    const bool tu[2] = {wave < NQu, wave + kWaves < NQu};   // this wave's u and v row tiles (wave-uniform)
    const bool tv[2] = {wave < NQv, wave + kWaves < NQv};
    int lcc[kKfMaxD / 16], zcc[kKfMaxD / 16], rcc[2][4];    // the coordinates this thread loads, clamped to dv - 1
#pragma unroll
    for (int j = 0; j < kKfMaxD / 16; ++j) {
        lcc[j] = lc + 16 * j < dv ? lc + 16 * j : dv - 1;
        zcc[j] = kf_pos(ls, Ku + lcc[j], Sz);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
            rcc[s][v] = r < dv ? r : dv - 1;
        }

    for (int e = t; e < 2 * 4 * kKfTile * kKfSz; e += kBlock) (&zs[0][0])[e] = 0.0f;
    for (int e = t; e < 4 * kKfTile * kKfS1; e += kBlock) {
        rs[e] = 0.0f;
        qs[e] = 0.0f;
    }
    __syncthreads();
    for (int c = lc; c < du; c += 16) zs[0][kf_pos(ls, c, Sz)] = d.m0[(size_t)lb * du + c];
    for (int c = lc; c < dv; c += 16) zs[0][kf_pos(ls, Ku + c, Sz)] = vsl[c];
    float *msl = nullptr, *rsl = nullptr;   // STORE: this lane's sample in st.ms and st.rs, advanced a step per step
    int dul = 0, dvl = 0;                   // the rows this lane stores: du and dv, none for a slot past the batch
    if constexpr (STORE) {
        if (blockIdx.x * kKfTile + ls < B)
            for (int c = lc; c < du; c += 16) st.ms[(size_t)lb * ((size_t)T + 1) * du + c] = d.m0[(size_t)lb * du + c];
        msl = st.ms + (size_t)bc * ((size_t)T + 1) * du;
        dul = live ? du : 0;
        dvl = live ? dv : 0;
        rsl = st.rs + (size_t)bc * (size_t)T * dv;
    }

    // operands of column group q of step k: H and Pm (phase 1), AK and W (phase 2), for this wave's row tiles
    // this lane's element of column group 0 of its first row tile, per table; a row tile is NQc * 64 float4 on, a step
    // NQr row tiles
    // NQr row tiles.  No load is predicated or branched round (the waits of a straight-line window are exact): a row
    // tile this wave does not have is row tile 0 again and a column group past the last is the last again, loaded and
    // not used.
    const int wu[2] = {tu[0] ? wave : 0, tu[1] ? wave + kWaves : 0}, wv[2] = {tv[0] ? wave : 0, tv[1] ? wave + kWaves : 0};
    const float4 *Hl[2], *Pl[2], *Al[2], *Wl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        Hl[s] = d.Hp + (size_t)wv[s] * NQz * 64 + lane;
        Pl[s] = d.Pp + (size_t)wu[s] * NQz * 64 + lane;
        Al[s] = d.AKp + (size_t)wu[s] * NQv * 64 + lane;
        Wl[s] = d.Wp + (size_t)wv[s] * NQv * 64 + lane;
    }
    const int sH = NQv * NQz * 64, sP = NQu * NQz * 64, sA = NQu * NQv * 64, sW = NQv * NQv * 64;   // float4 per step
    auto load1 = [&](int q, float4 (&h)[2], float4 (&pm)[2]) {
        const int qc = (q < NQz ? q : NQz - 1) * 64;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            h[s] = Hl[s][qc];
            pm[s] = Pl[s][qc];
        }
    };
    auto load2 = [&](int q, float4 (&ak)[2], float4 (&w)[2]) {
        const int qc = (q < NQv ? q : NQv - 1) * 64;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            ak[s] = Al[s][qc];
            w[s] = Wl[s][qc];
        }
    };
    // sum_i qv_i^2 of every sample of the tile as the diagonal of its Gram matrix (wave 0); lane smp + 16 (smp / 4) holds
    // its sample's sum in element smp % 4
    float ll = 0.0f;
    auto gram = [&](float lc_k) {
        mfma_f4 g = {0.0f, 0.0f, 0.0f, 0.0f};
        const float4* qb = reinterpret_cast<const float4*>(qs + lane * Sv);
        for (int q = 0; q < NQv; ++q) {
            const float4 x = qb[q];
            KF_MFMA4(g, x, x);
        }
        const int v = smp & 3;
        const float sum = v == 0 ? g[0] : (v == 1 ? g[1] : (v == 2 ? g[2] : g[3]));
        ll = ll + ((-0.5f * sum) + lc_k);
    };

    // the rolling windows, rings of kKfAhead + 1 slots: group q sits in slot q % (kKfAhead + 1), and the slot a group
    // has just left takes the group kKfAhead further on (no register in flight is ever copied: the loops are unrolled by
    // the ring size, so every slot index is a constant)
    float4 hr[kKfAhead + 1][2], pr[kKfAhead + 1][2], ar[kKfAhead + 1][2], wr[kKfAhead + 1][2];
#pragma unroll
    for (int i = 0; i <= kKfAhead; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) hr[i][s] = pr[i][s] = ar[i][s] = wr[i][s] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    mfma_f4 accP[2], accH[2], accW[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) accP[s] = accH[s] = accW[s] = mfma_f4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* el = d.ep + 4 * lg;   // this lane's rows of the biases of the step
    const float* cl = d.cp + 4 * lg;
    float4 bH[2], bP[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        bH[s] = *reinterpret_cast<const float4*>(el + 16 * wv[s]);
        bP[s] = *reinterpret_cast<const float4*>(cl + 16 * wu[s]);
    }
#pragma unroll
    for (int i = 0; i < kKfAhead; ++i) load1(i, hr[i], pr[i]);
    __syncthreads();

    int p = 0;
    for (int k = 0; k < T; ++k) {
        // the next observation: the loader's share of the next z tile and this lane's rows of the innovation.  No load
        // and no store is predicated: a coordinate past dv - 1 is dv - 1 again (the loader then stores the same value to
        // the same place twice; an innovation row past dv - 1 meets zero table columns only).
        float vn[kKfMaxD / 16], vr[2][4];
        vsl += dv;
        vsb += dv;
#pragma unroll
        for (int j = 0; j < kKfMaxD / 16; ++j) vn[j] = vsl[lcc[j]];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) vr[s][v] = vsb[rcc[s][v]];
#pragma unroll
        for (int i = 0; i < kKfAhead; ++i) load2(i, ar[i], wr[i]);
        const float lc_prev = d.lconst[k > 0 ? k - 1 : 0];
        if (k > 0 && wave == 0) gram(lc_prev);

        // phase 1: pred = e + H z and the part of m' that does not wait for the innovation, c + Pm z.  The biases came
        // a step ago; the next step's are asked for behind everything this step waits for (the counter of outstanding
        // loads is in order: waiting for a young load is waiting for every older one).
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            accH[s] = mfma_f4{bH[s].x, bH[s].y, bH[s].z, bH[s].w};
            accP[s] = mfma_f4{bP[s].x, bP[s].y, bP[s].z, bP[s].w};
        }
        const float4* zb = reinterpret_cast<const float4*>(zs[p] + lane * Sz);
        for (int q0 = 0; q0 < NQz; q0 += kKfAhead + 1) {
#pragma unroll
            for (int j = 0; j <= kKfAhead; ++j) {
                const int q = q0 + j;
                if (q >= NQz) break;
                load1(q + kKfAhead, hr[(j + kKfAhead) % (kKfAhead + 1)], pr[(j + kKfAhead) % (kKfAhead + 1)]);
                const float4 x = zb[q];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (tv[s]) KF_MFMA4(accH[s], hr[j][s], x);
                    if (tu[s]) KF_MFMA4(accP[s], pr[j][s], x);
                }
            }
        }
        // the first groups of the next step's first phase: in flight under the tails
        if (k + 1 < T) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                Hl[s] += sH;
                Pl[s] += sP;
            }
        }
#pragma unroll
        for (int i = 0; i < kKfAhead; ++i) load1(i, hr[i], pr[i]);
        if (k + 1 < T) {
            el += Kv;
            cl += Ku;
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bH[s] = *reinterpret_cast<const float4*>(el + 16 * wv[s]);
            bP[s] = *reinterpret_cast<const float4*>(cl + 16 * wu[s]);
        }
        // r_i = vs[k+1][i] - pred_i, and the observation half of the next z
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (tv[s]) {
#pragma unroll
                for (int v = 0; v < 4; ++v) rs[kf_pos(smp, 16 * (wave + kWaves * s) + 4 * lg + v, Sv)] = vr[s][v] - accH[s][v];
                if (STORE) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int r = kf_fresh(16 * (wave + kWaves * s) + 4 * lg + v);
                        if (r < dvl) rsl[r] = vr[s][v] - accH[s][v];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kKfMaxD / 16; ++j) zs[p ^ 1][zcc[j]] = vn[j];
        __syncthreads();

        // phase 2: m' continued over AK r, and qv = W r
#pragma unroll
        for (int s = 0; s < 2; ++s) accW[s] = mfma_f4{0.0f, 0.0f, 0.0f, 0.0f};
        const float4* rb = reinterpret_cast<const float4*>(rs + lane * Sv);
        for (int q0 = 0; q0 < NQv; q0 += kKfAhead + 1) {
#pragma unroll
            for (int j = 0; j <= kKfAhead; ++j) {
                const int q = q0 + j;
                if (q >= NQv) break;
                load2(q + kKfAhead, ar[(j + kKfAhead) % (kKfAhead + 1)], wr[(j + kKfAhead) % (kKfAhead + 1)]);
                const float4 x = rb[q];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (tu[s]) KF_MFMA4(accP[s], ar[j][s], x);
                    if (tv[s]) KF_MFMA4(accW[s], wr[j][s], x);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
                if (tu[s]) zs[p ^ 1][kf_pos(smp, r, Sz)] = accP[s][v];
                if (tv[s]) qs[kf_pos(smp, r, Sv)] = accW[s][v];
                if (STORE && tu[s] && kf_fresh(r) < dul) msl[du + r] = accP[s][v];
            }
        }
        if (STORE) {
            msl += du;
            rsl += dv;
        }
        __syncthreads();
        p ^= 1;
        if (k + 1 < T) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                Al[s] += sA;
                Wl[s] += sW;
            }
        }
    }
    if (wave == 0) {
        gram(d.lconst[T - 1]);
        if (loglik && live && lg == (smp >> 2)) loglik[b] = ll;
    }
    if (means) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
                if (tu[s] && live && r < du) means[(size_t)b * du + r] = accP[s][v];
            }
    }
    if (!DRAW) return;

    // x_j = m_T[j] + sum_c Lt[c][j] zz[c], zz = normal(key_kf, (du,)): the same product on the operand zz in the r tile
    const int Su = d.Su, half = (du + 1) >> 1;
    for (int e = t; e < 4 * kKfTile * kKfS1; e += kBlock) rs[e] = 0.0f;   // (its last reader is behind the loop's barrier)
    __syncthreads();
    uint32_t ka, kb;
    split_at(keys[2 * bc], keys[2 * bc + 1], 3, 2, ka, kb);                // key_kf of sample t % 16
    for (int i = t >> 4; i < half; i += kBlock / kKfTile) {
        uint32_t lo, hi;
        random_bits_pair_padded(ka, kb, (uint64_t)du, (uint64_t)i, lo, hi);
        rs[kf_pos(smp, i, Su)] = normal_from_bits(lo);
        if (i + half < du) rs[kf_pos(smp, i + half, Su)] = normal_from_bits(hi);
    }
    __syncthreads();
    const float4* xb = reinterpret_cast<const float4*>(rs + lane * Su);
    for (int q = 0; q < NQu; ++q) {
        const float4 x = xb[q];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (tu[s]) {
                const float4 a = d.Lp[((size_t)(wave + kWaves * s) * NQu + q) * 64 + lane];
                KF_MFMA4(accP[s], a, x);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
            if (tu[s] && live && r < du) samples[(size_t)b * du + r] = accP[s][v];
        }
}

// ---- the backward pass of the smoother and path sampler (fbsmi_kfs_*) ---------------------------------------------------
// delta_k = K[k] r_k + Lb[k] xi_k + J[k] delta_{k+1}, paths[k] = m_k + delta_k, k = T-1 .. 0, in k_kf's layout: a workgroup
// owns 16 samples (the MFMA columns) for all T steps, the u row tiles are dealt round-robin to the waves, the tables sit in
// the A-operand order of k_kf_pack.  delta is ping-ponged through LDS in the plane layout; r_k (the forward launch's) and
// xi[k] = normal(key_bwd, (T, du))[k] are staged into double-buffered operand tiles a step ahead, so the K r and Lb xi
// chains of step k - 1 run behind the barrier of step k, off the serial J delta path, whose operands are asked for a
// step ahead as well.  One barrier per step.  LDS: six tiles of 64 * 36 floats, 55 296 bytes, static.
struct KfsDev {
    int du, dv, T, NQu, NQv, Su, Sv;
    const float4 *Kp, *Jp, *Lbp;             // [T][NQu][NQv][64] [T][NQu][NQu][64] [T][NQu][NQu][64]
    const float *ms, *rs, *uT;               // [B][T+1][du] [B][T][dv] [B][du]
};

template <bool DRAW>
__global__ void __launch_bounds__(kBlock) k_kfs_back(KfsDev d, const uint32_t* __restrict__ keys, float* __restrict__ paths,
                                                     int B) {
    __shared__ __attribute__((aligned(16))) float ds[2][4 * kKfTile * kKfS1];
    __shared__ __attribute__((aligned(16))) float rl[2][4 * kKfTile * kKfS1];
    __shared__ __attribute__((aligned(16))) float xl[2][4 * kKfTile * kKfS1];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int du = d.du, dv = d.dv, T = d.T, NQu = d.NQu, NQv = d.NQv, Su = d.Su, Sv = d.Sv;
    const int smp = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x * kKfTile + smp;
    const bool live = b < B;
    const int bc = live ? b : B - 1;   // the slots past the batch repeat its last sample and store nothing
    const int dul = live ? du : 0;     // the rows this lane stores
    const int ls = t >> 4, lc = t & 15;   // the loader's view of the tile: sample t / 16, columns t % 16 + 16 j
    const bool llive = blockIdx.x * kKfTile + ls < B;
    const int lb = llive ? blockIdx.x * kKfTile + ls : B - 1;
    const bool tu[2] = {wave < NQu, wave + kWaves < NQu};
    const int wu[2] = {tu[0] ? wave : 0, tu[1] ? wave + kWaves : 0};
    const size_t T1 = (size_t)T + 1;
    const float* msb = d.ms + (size_t)bc * T1 * du;
    float* pb = paths + (size_t)bc * T1 * du;
    int rcl[2][4];                        // this lane's output rows, clamped to du - 1 for the loads of m_k
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
            rcl[s][v] = r < du ? r : du - 1;
        }

    for (int e = t; e < 2 * 4 * kKfTile * kKfS1; e += kBlock) {
        (&ds[0][0])[e] = 0.0f;
        (&rl[0][0])[e] = 0.0f;
        (&xl[0][0])[e] = 0.0f;
    }
    __syncthreads();
    // delta_T = u_T - m_T (DRAW; u_T is the forward launch's draw, stored as it is) or 0
    for (int c = lc; c < du; c += 16) {
        const float mT = d.ms[((size_t)lb * T1 + T) * du + c];
        if (DRAW) {
            const float uT = d.uT[(size_t)lb * du + c];
            ds[0][kf_pos(ls, c, Su)] = uT - mT;
            if (llive) paths[((size_t)lb * T1 + T) * du + c] = uT;
        } else {
            if (llive) paths[((size_t)lb * T1 + T) * du + c] = mT + 0.0f;
        }
    }
    uint32_t kb0 = 0, kb1 = 0;
    if (DRAW) split_at(keys[2 * lb], keys[2 * lb + 1], 3, 1, kb0, kb1);   // key_bwd of the loader's sample
    const uint64_t nxi = (uint64_t)kf_fresh(T) * du;   // (and what the draw derives from it: in vector registers)
    // r_k and xi[k] of the loader's sample into the operand tiles `buf`
    auto stage = [&](int k, int buf) {
        const float* rg = d.rs + ((size_t)lb * T + k) * dv;
        for (int c = lc; c < dv; c += 16) rl[buf][kf_pos(ls, c, Sv)] = rg[c];
        if (DRAW)
            for (int c = lc; c < du; c += 16) xl[buf][kf_pos(ls, c, Su)] = normal_at(kb0, kb1, nxi, (uint64_t)k * du + c);
    };
    // this lane's float4 of column group 0 of this wave's row tiles within a step's K and within its J or Lb (kept in
    // vector registers, like jo below)
    const int ko[2] = {kf_fresh(wu[0] * NQv * 64 + lane), kf_fresh(wu[1] * NQv * 64 + lane)};
    const int lo[2] = {kf_fresh(wu[0] * NQu * 64 + lane), kf_fresh(wu[1] * NQu * 64 + lane)};
    // acc = 0, then the K r_k chain, then the Lb xi_k chain, for this wave's row tiles
    mfma_f4 acc[2];
    auto ahead = [&](int k, int buf) {
        const float4* rb = reinterpret_cast<const float4*>(rl[buf] + lane * Sv);
        const float4* xb = reinterpret_cast<const float4*>(xl[buf] + lane * Su);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            acc[s] = mfma_f4{0.0f, 0.0f, 0.0f, 0.0f};
            if (!tu[s]) continue;
            const float4* Kl = d.Kp + (size_t)k * NQu * NQv * 64 + ko[s];
            for (int q = 0; q < NQv; ++q) {
                const float4 a = Kl[q * 64], x = rb[q];
                KF_MFMA4(acc[s], a, x);
            }
            if (DRAW) {
                const float4* Ll = d.Lbp + (size_t)k * NQu * NQu * 64 + lo[s];
                for (int q = 0; q < NQu; ++q) {
                    const float4 a = Ll[q * 64], x = xb[q];
                    KF_MFMA4(acc[s], a, x);
                }
            }
        }
    };
    // the J operands of a step, all of this wave's: asked for a step ahead.  No load is predicated: a row tile this wave
    // does not have is row tile 0 again and a column group past the last is the last again, loaded and not used.
    float4 jr[kKfMaxD / 16][2];
    int jo[kKfMaxD / 16];   // this lane's float4 of column group q (clamped) within a row tile: kept in vector registers
#pragma unroll
    for (int q = 0; q < kKfMaxD / 16; ++q) jo[q] = kf_fresh((q < NQu ? q : NQu - 1) * 64 + lane);
    auto loadJ = [&](int k) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float4* Jl = d.Jp + (size_t)k * NQu * NQu * 64 + (lo[s] - lane);
#pragma unroll
            for (int q = 0; q < kKfMaxD / 16; ++q) jr[q][s] = Jl[jo[q]];
        }
    };
    loadJ(T - 1);
    stage(T - 1, 0);
    __syncthreads();
    ahead(T - 1, 0);

    int p = 0;
    for (int k = T - 1; k >= 0; --k) {
        const int bk = (T - 1 - k) & 1;
        float mk[2][4];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) mk[s][v] = msb[(size_t)k * du + rcl[s][v]];
        if (k > 0) stage(k - 1, bk ^ 1);
        const float4* db = reinterpret_cast<const float4*>(ds[p] + lane * Su);
#pragma unroll
        for (int q = 0; q < kKfMaxD / 16; ++q) {
            if (q < NQu) {
                const float4 x = db[q];
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    if (tu[s]) KF_MFMA4(acc[s], jr[q][s], x);
            }
        }
        loadJ(k > 0 ? k - 1 : 0);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
                if (tu[s]) ds[p ^ 1][kf_pos(smp, r, Su)] = acc[s][v];
                if (tu[s] && kf_fresh(r) < dul) pb[(size_t)k * du + r] = mk[s][v] + acc[s][v];
            }
        __syncthreads();
        p ^= 1;
        if (k > 0) ahead(k - 1, bk ^ 1);
    }
}

}  // namespace

struct fbsmi_kf {
    KfDev d{};
    KfFront f{};
    int nsamples = 0;
    int front_block = 64;   // max(du, dv) rounded up to a wave
    bool has_fwd = false;   // F, sqQ are not all-zero placeholders
    void* pool = nullptr;
    bool em = false;        // fbsmi_kf_set_em_forward: the front of a sample call is k_kf_front_em
    KfEmFront e{};
    void* em_pool = nullptr;   // the prior's floats and the key slab
};

namespace {

// the front launch of a sample call
void kf_launch_front(fbsmi_kf* h, const uint32_t* keys, const float* y0, hipStream_t st) {
    const int B = h->nsamples;
    if (!h->em) k_kf_front<true><<<B, h->front_block, 0, st>>>(h->f, keys, y0, nullptr);
    else kf_front_em_launch(h->e, keys, y0, B, st);
}

}  // namespace

extern "C" {

int fbsmi_kf_create(const fbsmi_kf_model* m, int32_t nsamples, fbsmi_kf** out) {
    if (!out || !m || m->T < 1) return fail(FBSMI_ERR_ARG, "kf_create: need a model with T >= 1");
    if (!m->H || !m->e || !m->Pm || !m->c || !m->AK || !m->W || !m->lconst || !m->Lt || !m->F || !m->sqQ || !m->m_u ||
        !m->m_v || !m->gain)
        return fail(FBSMI_ERR_ARG, "kf_create: null table");
    if (m->du < 1 || m->du > kKfMaxD || m->dv < 1 || m->dv > kKfMaxD || nsamples < 1 || nsamples > 65535)
        return fail(FBSMI_ERR_UNSUPPORTED, "kf_create: the fused Kalman sampler takes 1 <= du, dv <= 128 and 1 <= nsamples <= 65535");
    const size_t T = m->T, du = m->du, dv = m->dv, D = du + dv, B = nsamples;
    bool any = false;
    {
        // a model whose forward process is Euler-Maruyama carries all-zero placeholders here (as in fbsmi_lg_fsamp_create)
        std::vector<float> F(T), Q(T);
        FBSMI_HIP_TRY(hipMemcpy(F.data(), m->F, sizeof(float) * T, hipMemcpyDeviceToHost));
        FBSMI_HIP_TRY(hipMemcpy(Q.data(), m->sqQ, sizeof(float) * T, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < T; ++k) any = any || F[k] != 0.0f || Q[k] != 0.0f;
    }
    fbsmi_kf* h = new (std::nothrow) fbsmi_kf();
    if (!h) return fail(FBSMI_ERR_ARG, "out of host memory");
    KfDev& d = h->d;
    const int NQu = (m->du + 15) / 16, NQv = (m->dv + 15) / 16, NQz = NQu + NQv;
    d.du = m->du; d.dv = m->dv; d.T = m->T; d.NQu = NQu; d.NQv = NQv;
    d.Sz = kf_plane_row(16 * NQz); d.Sv = kf_plane_row(16 * NQv); d.Su = kf_plane_row(16 * NQu);
    h->nsamples = nsamples;
    h->has_fwd = any;
    h->front_block = (m->du > 64 || m->dv > 64) ? kKfMaxD : 64;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t nH = T * NQv * NQz * 256, nP = T * NQu * NQz * 256, nAK = T * NQu * NQv * 256, nW = T * NQv * NQv * 256,
                 nL = (size_t)NQu * NQu * 256;
    const size_t o_H = take(nH * 4), o_P = take(nP * 4), o_AK = take(nAK * 4), o_W = take(nW * 4), o_L = take(nL * 4);
    const size_t o_e = take(T * 16 * NQv * 4), o_c = take(T * 16 * NQu * 4), o_lc = take(T * 4), o_F = take(T * 4), o_Q = take(T * 4);
    const size_t o_mu = take(du * 8), o_mv = take(dv * 8), o_g = take(du * dv * 8);
    const size_t o_vs = take(B * (T + 1) * dv * 4), o_m0 = take(B * du * 4);
    auto bail = [&](hipError_t e, const char* what) {
        const int rc = fail(FBSMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        fbsmi_kf_destroy(h);
        return rc;
    };
    hipError_t e;
    if ((e = hipMalloc(&h->pool, off)) != hipSuccess) return bail(e, "kf_create: hipMalloc");
    if ((e = hipMemset(h->pool, 0, off)) != hipSuccess) return bail(e, "kf_create: hipMemset");
    char* p = (char*)h->pool;
    d.Hp = (const float4*)(p + o_H); d.Pp = (const float4*)(p + o_P); d.AKp = (const float4*)(p + o_AK);
    d.Wp = (const float4*)(p + o_W); d.Lp = (const float4*)(p + o_L);
    d.ep = (const float*)(p + o_e); d.cp = (const float*)(p + o_c); d.lconst = (const float*)(p + o_lc);
    KfFront& f = h->f;
    f.du = m->du; f.dv = m->dv; f.T = m->T;
    f.F = (const float*)(p + o_F); f.sqQ = (const float*)(p + o_Q);
    f.m_u = (const double*)(p + o_mu); f.m_v = (const double*)(p + o_mv); f.gain = (const double*)(p + o_g);
    f.vs = (float*)(p + o_vs); f.m0 = (float*)(p + o_m0);
    d.m0 = f.m0;
    // the handle's own copies, made once
    const KfPack jobs[5] = {
        {m->H, (float*)(p + o_H), (int)T, (int)dv, (int)du, (int)dv, NQu, NQv, NQz, (int)D, 0, dv * D},
        {m->Pm, (float*)(p + o_P), (int)T, (int)du, (int)du, (int)dv, NQu, NQu, NQz, (int)D, 0, du * D},
        {m->AK, (float*)(p + o_AK), (int)T, (int)du, (int)dv, 0, NQv, NQu, NQv, (int)dv, 0, du * dv},
        {m->W, (float*)(p + o_W), (int)T, (int)dv, (int)dv, 0, NQv, NQv, NQv, (int)dv, 0, dv * dv},
        {m->Lt, (float*)(p + o_L), 1, (int)du, (int)du, 0, NQu, NQu, NQu, (int)du, 1, du * du},
    };
    const size_t counts[5] = {nH, nP, nAK, nW, nL};
    for (int i = 0; i < 5; ++i) {
        k_kf_pack<<<(unsigned)((counts[i] + kBlock - 1) / kBlock), kBlock, 0, nullptr>>>(jobs[i]);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e, "kf_create: pack launch");
    }
    k_kf_pad<<<(unsigned)((T * 16 * NQv + kBlock - 1) / kBlock), kBlock, 0, nullptr>>>(m->e, (float*)(p + o_e), (int)T, (int)dv, 16 * NQv);
    k_kf_pad<<<(unsigned)((T * 16 * NQu + kBlock - 1) / kBlock), kBlock, 0, nullptr>>>(m->c, (float*)(p + o_c), (int)T, (int)du, 16 * NQu);
    if ((e = hipGetLastError()) != hipSuccess) return bail(e, "kf_create: pad launch");
    const struct { size_t o; const void* src; size_t bytes; } copies[6] = {
        {o_lc, m->lconst, T * 4}, {o_F, m->F, T * 4}, {o_Q, m->sqQ, T * 4},
        {o_mu, m->m_u, du * 8}, {o_mv, m->m_v, dv * 8}, {o_g, m->gain, du * dv * 8}};
    for (const auto& cpy : copies)
        if ((e = hipMemcpy(p + cpy.o, cpy.src, cpy.bytes, hipMemcpyDeviceToDevice)) != hipSuccess) return bail(e, "kf_create: hipMemcpy");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "kf_create: pack");
    *out = h;
    return FBSMI_OK;
}

void fbsmi_kf_destroy(fbsmi_kf* h) {
    if (!h) return;
    if (h->pool) {
        (void)hipDeviceSynchronize();
        (void)hipFree(h->pool);
    }
    if (h->em_pool) (void)hipFree(h->em_pool);
    delete h;
}

int fbsmi_kf_set_em_forward(fbsmi_kf* h, const fbsmi_em_forward* f, const float* x0_mean, const float* x0_chol) {
    if (!h || !f || f->nsub < 1 || !f->M || !f->c || !f->ddt || !f->s)
        return fail(FBSMI_ERR_ARG, "kf_set_em_forward: need a handle and forward tables with nsub >= 1");
    if ((x0_mean == nullptr) != (x0_chol == nullptr))
        return fail(FBSMI_ERR_ARG, "kf_set_em_forward: x0_mean and x0_chol are both null or both set");
    if (h->has_fwd)
        return fail(FBSMI_ERR_UNSUPPORTED, "kf_set_em_forward: the model has an exact forward transition (F, sqQ)");
    const size_t du = h->d.du, T = h->d.T, B = h->nsamples;   // (du + dv <= 256 = kEmPathMaxD by kf_create's limits)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_mean = take(x0_mean ? du * 4 : 0), o_chol = take(x0_chol ? du * du * 4 : 0);
    const size_t o_keys = take((int)T > kKfEmKeysLds ? B * T * 2 * 4 : 0);
    void* pool = nullptr;
    if (off) {
        FBSMI_HIP_TRY(hipMalloc(&pool, off));
        hipError_t e = hipSuccess;
        if (x0_mean) {
            e = hipMemcpy((char*)pool + o_mean, x0_mean, du * 4, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy((char*)pool + o_chol, x0_chol, du * du * 4, hipMemcpyDeviceToDevice);
        }
        if (e != hipSuccess) {
            (void)hipFree(pool);
            return fail(FBSMI_ERR_HIP, std::string("kf_set_em_forward: hipMemcpy: ") + hipGetErrorString(e));
        }
    }
    if (h->em_pool) {   // set again: the launches that read the old copies are behind us
        (void)hipDeviceSynchronize();
        (void)hipFree(h->em_pool);
    }
    h->em_pool = pool;
    KfEmFront& e = h->e;
    e.du = h->f.du; e.dv = h->f.dv; e.T = h->f.T;
    e.nsub = f->nsub; e.M = f->M; e.c = f->c; e.ddt = f->ddt; e.s = f->s;
    e.x0_mean = x0_mean ? (const float*)((char*)pool + o_mean) : nullptr;
    e.x0_chol = x0_chol ? (const float*)((char*)pool + o_chol) : nullptr;
    e.ekeys = (int)T > kKfEmKeysLds ? (uint32_t*)((char*)pool + o_keys) : nullptr;
    e.m_u = h->f.m_u; e.m_v = h->f.m_v; e.gain = h->f.gain; e.vs = h->f.vs; e.m0 = h->f.m0;
    h->em = true;
    return FBSMI_OK;
}

int fbsmi_kf_sample(fbsmi_kf* h, const uint32_t* keys, const float* y0, float* samples, float* means, float* loglik,
                    void* stream) {
    if (!h || !keys || !y0 || !samples) return fail(FBSMI_ERR_ARG, "kf_sample: null argument");
    if (!h->has_fwd && !h->em)
        return fail(FBSMI_ERR_UNSUPPORTED, "kf_sample: the model has no exact forward transition (F, sqQ)");
    hipStream_t st = (hipStream_t)stream;
    const KfDev& d = h->d;
    const int B = h->nsamples;
    kf_launch_front(h, keys, y0, st);
    k_kf<true><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(d, h->f.vs, keys, samples, means, loglik, B, KfNoStore());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FBSMI_ERR_HIP, std::string("kf_sample launch: ") + hipGetErrorString(e));
    return FBSMI_OK;
}

int fbsmi_kf_filter(fbsmi_kf* h, const float* vs, float* means, float* loglik, void* stream) {
    if (!h || !vs) return fail(FBSMI_ERR_ARG, "kf_filter: null argument");
    hipStream_t st = (hipStream_t)stream;
    const KfDev& d = h->d;
    const int B = h->nsamples;
    k_kf_front<false><<<B, h->front_block, 0, st>>>(h->f, nullptr, nullptr, vs);
    k_kf<false><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(d, vs, nullptr, nullptr, means, loglik, B, KfNoStore());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FBSMI_ERR_HIP, std::string("kf_filter launch: ") + hipGetErrorString(e));
    return FBSMI_OK;
}

int fbsmi_kf_view(fbsmi_kf* h, int which, void* dst, int64_t* count, void* stream) {
    if (!h) return fail(FBSMI_ERR_ARG, "kf_view: null handle");
    const KfDev& d = h->d;
    const size_t B = h->nsamples;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = h->f.vs; n = B * ((size_t)d.T + 1) * d.dv; break;
        case 1: src = h->f.m0; n = B * d.du; break;
        default: return fail(FBSMI_ERR_ARG, "kf_view: which must be 0 (vs) or 1 (m_)");
    }
    if (count) *count = (int64_t)n;
    if (!dst || n == 0) return FBSMI_OK;
    FBSMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FBSMI_OK;
}

}  // extern "C"

// ---- fbsmi_kfs_*: the smoother and path sampler on top of a filter handle of its own ------------------------------------
struct fbsmi_kfs {
    fbsmi_kf* kf = nullptr;   // the front, the forward tables, vs and m_0
    KfsDev bd{};
    int nsamples = 0;
    void* pool = nullptr;
};

namespace {

// the forward launches of a call: the front, then the storing recursion (and the draw of u_T into the handle's buffer)
template <bool DRAW>
void kfs_forward(fbsmi_kfs* h, const float* vs, const uint32_t* keys, float* loglik, hipStream_t st) {
    const int B = h->nsamples;
    k_kf<DRAW, KfStore><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(
        h->kf->d, vs, keys, const_cast<float*>(h->bd.uT), nullptr, loglik, B,
        KfStore{const_cast<float*>(h->bd.ms), const_cast<float*>(h->bd.rs)});
}

}  // namespace

extern "C" {

int fbsmi_kfs_create(const fbsmi_kfs_model* m, int32_t nsamples, fbsmi_kfs** out) {
    if (!out || !m || !m->kf || m->kf->T < 1) return fail(FBSMI_ERR_ARG, "kfs_create: need a model with T >= 1");
    const fbsmi_kf_model* f = m->kf;
    if (!f->H || !f->e || !f->Pm || !f->c || !f->AK || !f->W || !f->lconst || !f->Lt || !f->F || !f->sqQ || !f->m_u || !f->m_v ||
        !f->gain || !m->K || !m->J || !m->Lb)
        return fail(FBSMI_ERR_ARG, "kfs_create: null table");
    if (f->du < 1 || f->du > kKfMaxD || f->dv < 1 || f->dv > kKfMaxD || nsamples < 1 || nsamples > 65535)
        return fail(FBSMI_ERR_UNSUPPORTED,
                    "kfs_create: the fused Kalman smoother takes 1 <= du, dv <= 128 and 1 <= nsamples <= 65535");
    fbsmi_kfs* h = new (std::nothrow) fbsmi_kfs();
    if (!h) return fail(FBSMI_ERR_ARG, "out of host memory");
    int rc = fbsmi_kf_create(f, nsamples, &h->kf);
    if (rc != FBSMI_OK) {
        delete h;
        return rc;
    }
    const size_t T = f->T, du = f->du, dv = f->dv, B = nsamples;
    const int NQu = h->kf->d.NQu, NQv = h->kf->d.NQv;
    h->nsamples = nsamples;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t nK = T * NQu * NQv * 256, nJ = T * NQu * NQu * 256;
    const size_t o_K = take(nK * 4), o_J = take(nJ * 4), o_L = take(nJ * 4);
    const size_t o_ms = take(B * (T + 1) * du * 4), o_rs = take(B * T * dv * 4), o_uT = take(B * du * 4);
    auto bail = [&](hipError_t e, const char* what) {
        const int r = fail(FBSMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        fbsmi_kfs_destroy(h);
        return r;
    };
    hipError_t e;
    if ((e = hipMalloc(&h->pool, off)) != hipSuccess) return bail(e, "kfs_create: hipMalloc");
    if ((e = hipMemset(h->pool, 0, off)) != hipSuccess) return bail(e, "kfs_create: hipMemset");
    char* p = (char*)h->pool;
    KfsDev& bd = h->bd;
    bd.du = f->du; bd.dv = f->dv; bd.T = f->T; bd.NQu = NQu; bd.NQv = NQv; bd.Su = h->kf->d.Su; bd.Sv = h->kf->d.Sv;
    bd.Kp = (const float4*)(p + o_K); bd.Jp = (const float4*)(p + o_J); bd.Lbp = (const float4*)(p + o_L);
    bd.ms = (const float*)(p + o_ms); bd.rs = (const float*)(p + o_rs); bd.uT = (const float*)(p + o_uT);
    const KfPack jobs[3] = {
        {m->K, (float*)(p + o_K), (int)T, (int)du, (int)dv, 0, NQv, NQu, NQv, (int)dv, 0, du * dv},
        {m->J, (float*)(p + o_J), (int)T, (int)du, (int)du, 0, NQu, NQu, NQu, (int)du, 0, du * du},
        {m->Lb, (float*)(p + o_L), (int)T, (int)du, (int)du, 0, NQu, NQu, NQu, (int)du, 0, du * du},
    };
    const size_t counts[3] = {nK, nJ, nJ};
    for (int i = 0; i < 3; ++i) {
        k_kf_pack<<<(unsigned)((counts[i] + kBlock - 1) / kBlock), kBlock, 0, nullptr>>>(jobs[i]);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e, "kfs_create: pack launch");
    }
    if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "kfs_create: pack");
    *out = h;
    return FBSMI_OK;
}

void fbsmi_kfs_destroy(fbsmi_kfs* h) {
    if (!h) return;
    if (h->pool) {
        (void)hipDeviceSynchronize();
        (void)hipFree(h->pool);
    }
    fbsmi_kf_destroy(h->kf);
    delete h;
}

static int kfs_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FBSMI_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return FBSMI_OK;
}

int fbsmi_kfs_set_em_forward(fbsmi_kfs* h, const fbsmi_em_forward* f, const float* x0_mean, const float* x0_chol) {
    if (!h || !f || f->nsub < 1 || !f->M || !f->c || !f->ddt || !f->s)
        return fail(FBSMI_ERR_ARG, "kfs_set_em_forward: need a handle and forward tables with nsub >= 1");
    if ((x0_mean == nullptr) != (x0_chol == nullptr))
        return fail(FBSMI_ERR_ARG, "kfs_set_em_forward: x0_mean and x0_chol are both null or both set");
    return fbsmi_kf_set_em_forward(h->kf, f, x0_mean, x0_chol);
}

int fbsmi_kfs_sample(fbsmi_kfs* h, const uint32_t* keys, const float* y0, float* paths, float* loglik, void* stream) {
    if (!h || !keys || !y0 || !paths) return fail(FBSMI_ERR_ARG, "kfs_sample: null argument");
    if (!h->kf->has_fwd && !h->kf->em)
        return fail(FBSMI_ERR_UNSUPPORTED, "kfs_sample: the model has no exact forward transition (F, sqQ)");
    hipStream_t st = (hipStream_t)stream;
    const int B = h->nsamples;
    kf_launch_front(h->kf, keys, y0, st);
    kfs_forward<true>(h, h->kf->f.vs, keys, loglik, st);
    k_kfs_back<true><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(h->bd, keys, paths, B);
    return kfs_launched("kfs_sample");
}

int fbsmi_kfs_sample_on(fbsmi_kfs* h, const uint32_t* keys, const float* vs, float* paths, float* loglik, void* stream) {
    if (!h || !keys || !vs || !paths) return fail(FBSMI_ERR_ARG, "kfs_sample_on: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int B = h->nsamples;
    k_kf_front<false><<<B, h->kf->front_block, 0, st>>>(h->kf->f, nullptr, nullptr, vs);
    kfs_forward<true>(h, vs, keys, loglik, st);
    k_kfs_back<true><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(h->bd, keys, paths, B);
    return kfs_launched("kfs_sample_on");
}

int fbsmi_kfs_smooth(fbsmi_kfs* h, const float* vs, float* smeans, float* loglik, void* stream) {
    if (!h || !vs || !smeans) return fail(FBSMI_ERR_ARG, "kfs_smooth: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int B = h->nsamples;
    k_kf_front<false><<<B, h->kf->front_block, 0, st>>>(h->kf->f, nullptr, nullptr, vs);
    kfs_forward<false>(h, vs, nullptr, loglik, st);
    k_kfs_back<false><<<(B + kKfTile - 1) / kKfTile, kBlock, 0, st>>>(h->bd, nullptr, smeans, B);
    return kfs_launched("kfs_smooth");
}

int fbsmi_kfs_view(fbsmi_kfs* h, int which, void* dst, int64_t* count, void* stream) {
    if (!h) return fail(FBSMI_ERR_ARG, "kfs_view: null handle");
    const size_t B = h->nsamples, T = h->bd.T;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = h->kf->f.vs; n = B * (T + 1) * h->bd.dv; break;
        case 1: src = h->bd.ms; n = B * (T + 1) * h->bd.du; break;
        case 2: src = h->bd.rs; n = B * T * h->bd.dv; break;
        default: return fail(FBSMI_ERR_ARG, "kfs_view: which must be 0 (vs), 1 (filter means) or 2 (innovations)");
    }
    if (count) *count = (int64_t)n;
    if (!dst || n == 0) return FBSMI_OK;
    FBSMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FBSMI_OK;
}

}  // extern "C"

#undef KF_MFMA4
