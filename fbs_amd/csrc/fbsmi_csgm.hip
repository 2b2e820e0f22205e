// fbsmi_csgm.hip -- fused, batched conditional score sampler (Song et al., 2021; experiments/toy/gp_csgm.py) for the
// analytic Gaussian model (include/fbsmi.h, fbsmi_csgm_*).
//
// Both scores of the model are Gaussian, so the reverse drift is affine, f(x) = A[k] x + cvec[k], and a conditional sample
// is u0 = m_ref + S_ref z followed by T Euler-Maruyama steps.  The trajectories are independent: a whole batch is ONE
// launch of k_csgm, no key, init or per-step launches, no graph.
//
// A workgroup (4 waves) owns 16 samples for the whole trajectory.  The samples are the 16 columns of
// v_mfma_f32_16x16x4_f32 (which accumulates as an ascending fmaf chain, bit for bit: tools/mfmatest.hip), the table rows
// its 16 rows; the NQ = ceil(d / 16) row tiles are dealt round-robin to the waves (row tile w, w + 4 on wave w).
//   * Tables.  fbsmi_csgm_create repacks S_ref (table 0) and A[0..T-1] (tables 1..T) once into the lane order of the
//     A operand, zero-padded to NQ * 16 rows and columns: one coalesced 16-byte load per lane is the operand of four
//     consecutive MFMAs, rows and columns >= d contribute exactly +0 and no address needs a clamp.  The table of the next
//     step is fetched to registers while the current step's dependent chain of 4 NQ MFMAs runs.
//   * State.  The lane that holds accumulator element (row, sample) holds x[sample][row] in a register for the whole
//     trajectory; the copy the other waves multiply with sits in LDS in the plane layout of fbsmi_lg.hip's wide_pos
//     (lane l reads its four-MFMA operand as one ds_read_b128 at l * S + 4 q), ping-ponged: one barrier per step.
//   * Noise.  xi of step k + 1 is drawn under step k's product into an LDS tile: thread t serves sample t % 16 and the
//     pairs (i, i + half), i = t / 16, t / 16 + 16, ..., one Threefry call per pair; the step keys split(key_sde, T)[k]
//     are one more call per wave, the two words exchanged by lane shuffles.
//   * u0 is formed by the same product code: z = normal(key_init, (d,)) is the operand, S_ref the table, m_ref the bias.
// LDS: 2 x-tiles of 64 S floats (S <= 36) and 2 noise tiles of 16 (16 NQ + 4) floats, 35 328 bytes at d = 128, static.
#include <new>

#include "../../include/fbsmi.h"
#include "fbsmi_device.h"
#include "fbsmi_host.h"

using namespace fbsmi;

namespace {

constexpr int kCsTile = 16;          // samples per workgroup
constexpr int kCsMaxQ = 8;           // row tiles at d = 128
constexpr int kCsMaxS = 36;          // cs_plane_row(128)
constexpr int kCsMaxZ = 16 * kCsMaxQ + 4;
typedef float mfma_f4 __attribute__((ext_vector_type(4)));

struct CsgmDev {
    int d, T, S;
    const float4* Ap;   // [T+1][NQ][NQ][64]  table t, row tile, column group, lane: the A operand of four MFMAs
    const float* bp;    // [T+1][16 NQ]       m_ref, cvec[0..T-1], zero padded
    const float* ddt;   // [T]
    const float* s;     // [T]
    float* u0;          // [B][d]
    float* path;        // [T+1][B][d], nullable
};

// wide_pos of fbsmi_lg.hip for a 16-row tile: element (sample i, column c), S floats per plane row
__device__ __forceinline__ int cs_pos(int i, int c, int S) { return ((c & 3) * kCsTile + i) * S + (c >> 2); }
inline int cs_plane_row(int Kp) { return ((Kp / 4) & 4) ? Kp / 4 : Kp / 4 + 4; }

// table (t < 0: nothing), row r < d, column c < d of the caller's model
struct CsgmSrc {
    const float *A, *cvec, *m_ref, *S_ref;
};

// one thread per float of the packed tables; rows and columns >= d are zero
__global__ void __launch_bounds__(kBlock) k_csgm_pack(CsgmSrc m, int D, int T, int NQ, float* Ap, float* bp) {
    const size_t per = (size_t)NQ * NQ * 256, total = (size_t)(T + 1) * per;
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e < total) {
        const int t = (int)(e / per);
        const int w = (int)(e - (size_t)t * per);
        const int mm = w & 3, l = (w >> 2) & 63, q = (w >> 8) % NQ, rt = (w >> 8) / NQ;
        const int r = 16 * rt + (l & 15), c = 16 * q + 4 * mm + (l >> 4);
        float v = 0.0f;
        if (r < D && c < D) v = t == 0 ? m.S_ref[(size_t)r * D + c] : m.A[((size_t)(t - 1) * D + r) * D + c];
        Ap[e] = v;
    }
    const int Kp = 16 * NQ;
    if (e < (size_t)(T + 1) * Kp) {
        const int t = (int)(e / Kp), r = (int)(e - (size_t)t * Kp);
        float v = 0.0f;
        if (r < D) v = t == 0 ? m.m_ref[r] : m.cvec[(size_t)(t - 1) * D + r];
        bp[e] = v;
    }
}

template <int NQ>
__global__ void __launch_bounds__(kBlock) k_csgm(CsgmDev d, const uint32_t* __restrict__ keys, const float* __restrict__ u0in,
                                                 float* __restrict__ out, int B) {
    constexpr int NS = (NQ + kWaves - 1) / kWaves;   // row tiles per wave
    constexpr int ZS = 16 * NQ + 4;                  // floats per sample of a noise tile
    __shared__ __attribute__((aligned(16))) float xs[2][4 * kCsTile * kCsMaxS];
    __shared__ __attribute__((aligned(16))) float zs[2][kCsTile * kCsMaxZ];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int D = d.d, T = d.T, S = d.S;
    const int smp = lane & 15, lg = lane >> 4;
    const int b = blockIdx.x * kCsTile + smp;
    const bool live = b < B;
    const int bc = live ? b : B - 1;   // the slots past the batch repeat its last sample and store nothing
    const int half = (D + 1) >> 1;

    // keys: sample mode key_init, key_sde = split(keys[b], 2); integrate mode keys[b] is key_sde
    uint32_t k0 = keys[2 * bc], k1 = keys[2 * bc + 1], i0 = 0, i1 = 0;
    if (!u0in) {
        uint32_t s0, s1;
        split_at(k0, k1, 2, 0, i0, i1);
        split_at(k0, k1, 2, 1, s0, s1);
        k0 = s0;
        k1 = s1;
    }
    // split(key_sde, T)[k]: lanes 0-15 and 32-47 compute word 0, lanes 16-31 and 48-63 word 1 of their sample's key
    auto step_key = [&](int k, uint32_t& a, uint32_t& bb) {
        const uint32_t w = random_bits_at(k0, k1, 2ull * T, 2ull * k + (lg & 1));
        a = (uint32_t)__shfl((int)w, smp);
        bb = (uint32_t)__shfl((int)w, 16 + smp);
    };
    // normal(key, (d,)) of this thread's sample, the pairs (i, i + half) of this thread, to dst through pos(sample, i)
    auto draw = [&](uint32_t a, uint32_t bb, float* dst, auto pos) {
        for (int i = t >> 4; i < half; i += kBlock / kCsTile) {
            uint32_t lo, hi;
            random_bits_pair_padded(a, bb, (uint64_t)D, (uint64_t)i, lo, hi);
            dst[pos(smp, i)] = normal_from_bits(lo);
            if (i + half < D) dst[pos(smp, i + half)] = normal_from_bits(hi);
        }
    };
    auto zpos = [&](int i, int c) { return i * ZS + c; };
    auto xpos = [&](int i, int c) { return cs_pos(i, c, S); };

    for (int e = t; e < 2 * 4 * kCsTile * kCsMaxS; e += kBlock) (&xs[0][0])[e] = 0.0f;
    for (int e = t; e < 2 * kCsTile * kCsMaxZ; e += kBlock) (&zs[0][0])[e] = 0.0f;
    __syncthreads();

    // this lane's accumulator rows: row tile rt[s] = wave + 4 s, rows 16 rt + 4 lg + v
    float4 acur[NS][NQ], anxt[NS][NQ], bias[NS], bnxt[NS];
    float x[NS][4];
    const size_t tab = (size_t)NQ * NQ * 64;
    auto fetch = [&](int tt, float4 (&a)[NS][NQ], float4 (&bv)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int rt = wave + kWaves * s;
            if (rt < NQ) {   // wave-uniform
#pragma unroll
                for (int q = 0; q < NQ; ++q) a[s][q] = d.Ap[(size_t)tt * tab + ((size_t)rt * NQ + q) * 64 + lane];
                bv[s] = *reinterpret_cast<const float4*>(d.bp + (size_t)tt * (16 * NQ) + 16 * rt + 4 * lg);
            }
        }
    };
    // acc = bias_r, then acc = fma(M[r][c], x[c], acc) for c ascending, on the matrix cores
    auto product = [&](const float4 (&a)[NS][NQ], const float4 (&bv)[NS], const float* xt, mfma_f4 (&acc)[NS]) {
        const float4* xb = reinterpret_cast<const float4*>(xt + lane * S);
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = mfma_f4{bv[s].x, bv[s].y, bv[s].z, bv[s].w};
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float4 xv = xb[q];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (wave + kWaves * s < NQ) {
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][q].x, xv.x, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][q].y, xv.y, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][q].z, xv.z, acc[s], 0, 0, 0);
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][q].w, xv.w, acc[s], 0, 0, 0);
                }
            }
        }
    };
    // x of this lane to the LDS tile the next product reads, to global row `g` (nullable) of a (., B, d) array
    auto publish = [&](float* xt, float* g) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int rt = wave + kWaves * s;
            if (rt < NQ) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = 16 * rt + 4 * lg + v;
                    xt[cs_pos(smp, r, S)] = x[s][v];
                    if (g && live && r < D) g[(size_t)b * D + r] = x[s][v];
                }
            }
        }
    };

    fetch(u0in ? 1 : 0, acur, bias);
    uint32_t ka, kb;
    step_key(0, ka, kb);
    draw(ka, kb, zs[0], zpos);
    if (!u0in) {
        // u0_i = m_ref_i + sum_c S_ref[i][c] z_c: the product on the operand z
        draw(i0, i1, xs[0], xpos);
        __syncthreads();
        mfma_f4 acc[NS];
        product(acur, bias, xs[0], acc);
        fetch(1, acur, bias);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) x[s][v] = acc[s][v];
    } else {
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int r = 16 * (wave + kWaves * s) + 4 * lg + v;
                x[s][v] = u0in[(size_t)bc * D + (r < D ? r : 0)];
                if (r >= D) x[s][v] = 0.0f;
            }
    }
    publish(xs[1], d.u0);
    if (d.path) publish(xs[1], d.path);
    float h_n = d.ddt[0], s_n = d.s[0];
    __syncthreads();

    int p = 1;
    for (int k = 0; k < T; ++k) {
        const float h = h_n, sk = s_n;
        const int k1 = k + 1 < T ? k + 1 : k;
        fetch(k1 + 1, anxt, bnxt);   // the next step's table and bias: in flight under this step's chain
        h_n = d.ddt[k1];
        s_n = d.s[k1];
        mfma_f4 acc[NS];
        product(acur, bias, xs[p], acc);
        if (k + 1 < T) {             // the next step's noise (uniform branch)
            step_key(k + 1, ka, kb);
            draw(ka, kb, zs[(k + 1) & 1], zpos);
        }
        // x_i = (x_i + f_i * ddt[k]) + s[k] * xi_i
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int rt = wave + kWaves * s;
            if (rt < NQ) {
                const float4 z = *reinterpret_cast<const float4*>(&zs[k & 1][smp * ZS + 16 * rt + 4 * lg]);
                x[s][0] = (x[s][0] + acc[s][0] * h) + sk * z.x;
                x[s][1] = (x[s][1] + acc[s][1] * h) + sk * z.y;
                x[s][2] = (x[s][2] + acc[s][2] * h) + sk * z.z;
                x[s][3] = (x[s][3] + acc[s][3] * h) + sk * z.w;
            }
        }
        publish(xs[p ^ 1], k + 1 == T ? out : (d.path ? d.path + (size_t)(k + 1) * B * D : nullptr));
        if (k + 1 == T && d.path) publish(xs[p ^ 1], d.path + (size_t)T * B * D);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) acur[s][q] = anxt[s][q];
            bias[s] = bnxt[s];
        }
        __syncthreads();
        p ^= 1;
    }
}

template <int NQ>
void csgm_launch(const CsgmDev& d, const uint32_t* keys, const float* u0, float* out, int B, hipStream_t st) {
    k_csgm<NQ><<<(B + kCsTile - 1) / kCsTile, kBlock, 0, st>>>(d, keys, u0, out, B);
}

}  // namespace

struct fbsmi_csgm {
    CsgmDev d{};
    int nsamples = 0;
    void* pool = nullptr;
};

extern "C" {

int fbsmi_csgm_create(const fbsmi_csgm_model* m, int32_t nsamples, int store_path, fbsmi_csgm** out) {
    if (!out || !m || m->T < 1) return fail(FBSMI_ERR_ARG, "csgm_create: need a model with T >= 1");
    if (!m->A || !m->cvec || !m->ddt || !m->s || !m->m_ref || !m->S_ref) return fail(FBSMI_ERR_ARG, "csgm_create: null table");
    if (m->d < 1 || m->d > 128 || nsamples < 1 || nsamples > 131072)
        return fail(FBSMI_ERR_UNSUPPORTED, "csgm_create: the fused CSGM takes 1 <= d <= 128 and 1 <= nsamples <= 131072");
    fbsmi_csgm* h = new (std::nothrow) fbsmi_csgm();
    if (!h) return fail(FBSMI_ERR_ARG, "out of host memory");
    CsgmDev& d = h->d;
    const int NQ = (m->d + 15) / 16, Kp = 16 * NQ;
    d.d = m->d; d.T = m->T; d.S = cs_plane_row(Kp);
    h->nsamples = nsamples;
    const size_t B = nsamples, D = m->d, T = m->T;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t nAp = (T + 1) * (size_t)NQ * NQ * 256;
    const size_t o_Ap = take(nAp * 4), o_bp = take((T + 1) * Kp * 4), o_ddt = take(T * 4), o_s = take(T * 4), o_u0 = take(B * D * 4);
    const size_t o_path = store_path ? take((T + 1) * B * D * 4) : 0;
    auto bail = [&](hipError_t e, const char* what) {
        const int rc = fail(FBSMI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
        fbsmi_csgm_destroy(h);
        return rc;
    };
    hipError_t e;
    if ((e = hipMalloc(&h->pool, off)) != hipSuccess) return bail(e, "csgm_create: hipMalloc");
    if ((e = hipMemset(h->pool, 0, off)) != hipSuccess) return bail(e, "csgm_create: hipMemset");
    char* p = (char*)h->pool;
    d.Ap = (const float4*)(p + o_Ap); d.bp = (const float*)(p + o_bp); d.ddt = (const float*)(p + o_ddt); d.s = (const float*)(p + o_s);
    d.u0 = (float*)(p + o_u0);
    d.path = store_path ? (float*)(p + o_path) : nullptr;
    // the handle's own copies, made once: the packed tables, ddt and s
    const CsgmSrc src{m->A, m->cvec, m->m_ref, m->S_ref};
    k_csgm_pack<<<(unsigned)((nAp + kBlock - 1) / kBlock), kBlock, 0, nullptr>>>(src, m->d, m->T, NQ, (float*)(p + o_Ap), (float*)(p + o_bp));
    if ((e = hipGetLastError()) != hipSuccess) return bail(e, "csgm_create: pack launch");
    if ((e = hipMemcpy(p + o_ddt, m->ddt, T * 4, hipMemcpyDeviceToDevice)) != hipSuccess) return bail(e, "csgm_create: hipMemcpy");
    if ((e = hipMemcpy(p + o_s, m->s, T * 4, hipMemcpyDeviceToDevice)) != hipSuccess) return bail(e, "csgm_create: hipMemcpy");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "csgm_create: pack");
    *out = h;
    return FBSMI_OK;
}

void fbsmi_csgm_destroy(fbsmi_csgm* h) {
    if (!h) return;
    if (h->pool) {
        (void)hipDeviceSynchronize();
        (void)hipFree(h->pool);
    }
    delete h;
}

int fbsmi_csgm_run(fbsmi_csgm* h, const uint32_t* keys, const float* u0, float* out, void* stream) {
    if (!h || !keys || !out) return fail(FBSMI_ERR_ARG, "csgm_run: null input");
    const int nbatch = h->nsamples;
    hipStream_t st = (hipStream_t)stream;
    const CsgmDev& d = h->d;
    switch ((d.d + 15) / 16) {
        case 1: csgm_launch<1>(d, keys, u0, out, nbatch, st); break;
        case 2: csgm_launch<2>(d, keys, u0, out, nbatch, st); break;
        case 3: csgm_launch<3>(d, keys, u0, out, nbatch, st); break;
        case 4: csgm_launch<4>(d, keys, u0, out, nbatch, st); break;
        case 5: csgm_launch<5>(d, keys, u0, out, nbatch, st); break;
        case 6: csgm_launch<6>(d, keys, u0, out, nbatch, st); break;
        case 7: csgm_launch<7>(d, keys, u0, out, nbatch, st); break;
        default: csgm_launch<8>(d, keys, u0, out, nbatch, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FBSMI_ERR_HIP, std::string("csgm launch: ") + hipGetErrorString(e));
    return FBSMI_OK;
}

int fbsmi_csgm_view(fbsmi_csgm* h, int which, void* dst, int64_t* count, void* stream) {
    if (!h) return fail(FBSMI_ERR_ARG, "csgm_view: null handle");
    const CsgmDev& d = h->d;
    const size_t B = h->nsamples, D = d.d, T = d.T;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = d.u0; n = B * D; break;
        case 1:
            if (!d.path) return fail(FBSMI_ERR_ARG, "csgm_view: the handle was created without store_path");
            src = d.path; n = (T + 1) * B * D; break;
        default: return fail(FBSMI_ERR_ARG, "csgm_view: which must be 0 (u0) or 1 (path)");
    }
    if (count) *count = (int64_t)n;
    if (!dst || n == 0) return FBSMI_OK;
    FBSMI_HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return FBSMI_OK;
}

}  // extern "C"
