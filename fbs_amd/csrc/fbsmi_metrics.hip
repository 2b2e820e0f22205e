// fbsmi_metrics.hip -- image-quality metrics on the device (include/fbsmi.h, "image metrics"): PSNR and SSIM of a block
// of restored images against their true images, and the per-variable autocorrelation of image chains with its
// best-variable curve.  All statistics are float64; the inputs are float32 and their products are exact in float64.
//
// PSNR / SSIM.  A workgroup of 256 threads scores one band of rows of one channel of one restored image:
//   grid.x = (image * C + channel) * nb + band.
// The band's rows of both planes sit in LDS as float32 (they are read 14 times each).  The 7x7 window sums of the five
// quantities x, y, xx, yy, xy are separable: a thread owns one column of a segment of the band's rows and keeps the five
// 7-row column sums as running sums (one row enters, one leaves per step); the column sums of a step go to LDS as
// float64 and the thread of the window's left column adds seven of them.  A running sum is restarted from a direct sum at
// the top of every segment, so it drifts over at most a band's rows.
//
// LDS layout of a workgroup (dynamic, sized by the host for the image's width W and band height):
//   double cs[5][nseg * W]      column sums of the step, quantity-major: consecutive threads write and read consecutive
//                               doubles, so the 8-byte accesses are conflict-free; nseg * W <= 256, 10 KiB at the most
//   float  px[rin * W]          the true image's band, rin = rows per band + 6
//   float  py[rin * W]          the restored image's band
// The host chooses the band so that the two planes take at most 48 KiB (rin <= 6144 / W rows): 58 KiB with the column
// sums, under the 64 KiB a workgroup gets without asking for more; a 28 x 28 plane takes 6 KiB and 16 KiB in all, so ten
// workgroups share a compute unit's 160 KiB.  The tree reductions at the end reuse cs.
//
// Every sum has a fixed order that depends on (H, W, C) alone: a thread's windows top to bottom, the 256 threads by a
// binary tree in LDS, the bands and channels in index order in k_psnr_ssim_finish.  No atomics.
//
// Autocorrelation.  k_autocorr: a thread per variable d of a chain (loads coalesced across d), the mean, the centred
// variance and every lag as a direct float64 sum over t ascending.  k_autocorr_best: a workgroup per (chain, lag) takes
// the minimum over the non-constant variables of max(ac, 0) -- a minimum of non-negative numbers, so its value does not
// depend on the order, which is fixed anyway (strided per thread, then the binary tree).  gfx950 only.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fbsmi.h"
#include "fbsmi_host.h"

namespace fbsmi {

namespace {

constexpr int kBlock = 256;
constexpr int kWin = 7;                    // SSIM window
constexpr int kPlaneFloats = 6144;         // floats of one staged plane: 24 rows of 256, or a whole 64 x 96 image
constexpr int64_t kMaxGrid = 2147483647LL;

#define FBSMI_NEED(cond, msg) \
    if (!(cond)) return fail(FBSMI_ERR_ARG, msg)
#define FBSMI_LAUNCH_CHECK()                                                 \
    do {                                                                         \
        hipError_t e_ = hipGetLastError();                                       \
        if (e_ != hipSuccess) return fail(FBSMI_ERR_HIP, hipGetErrorString(e_)); \
    } while (0)

struct Bands {
    int nb;      // bands of an image
    int rpb;     // window rows of a band (the last may have fewer, or none)
    int nseg;    // row segments of a band that advance side by side
    int rps;     // window rows of a segment
};

// depends on (H, W) alone
Bands bands_for(int H, int W) {
    Bands b;
    const int hout = H - (kWin - 1);
    int rin = kPlaneFloats / W;
    if (rin > 256) rin = 256;
    const int bo = rin - (kWin - 1);       // >= 18
    b.nb = (hout + bo - 1) / bo;
    b.rpb = (hout + b.nb - 1) / b.nb;
    b.nseg = kBlock / W;
    b.rps = (b.rpb + b.nseg - 1) / b.nseg;
    return b;
}

// binary tree over a[0, 256); every thread of the workgroup calls it; the sum is in a[0] afterwards
__device__ __forceinline__ void tree256(double* a) {
    for (int s = kBlock / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) a[threadIdx.x] = a[threadIdx.x] + a[threadIdx.x + s];
    }
    __syncthreads();
}

__device__ __forceinline__ float clip01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// part[(image * C + channel) * nb + band] = {sum of the SSIM map over the band's windows, sum of squared differences over
// the rows the band owns}
__global__ void __launch_bounds__(kBlock) k_psnr_ssim_band(const float* __restrict__ tru, const float* __restrict__ res,
                                                           int S, int H, int W, int C, int clip, Bands bd,
                                                           double* __restrict__ part) {
    extern __shared__ double lds_d[];
    const int tid = threadIdx.x;
    const int band = blockIdx.x % bd.nb;
    const int ic = blockIdx.x / bd.nb;
    const int c = ic % C;
    const int64_t img = ic / C;
    const int hout = H - (kWin - 1), wout = W - (kWin - 1);
    int r0 = band * bd.rpb;
    if (r0 > hout) r0 = hout;
    int r1 = r0 + bd.rpb;
    if (r1 > hout) r1 = hout;
    const int rend = (band == bd.nb - 1) ? H : r1 + (kWin - 1);      // rows [r0, rend) are staged
    const int own_end = (band == bd.nb - 1) ? H : r1;                // rows [r0, own_end) count for the squared error
    const int ncs = bd.nseg * W;
    double* cs = lds_d;
    float* px = reinterpret_cast<float*>(lds_d + 5 * ncs);
    float* py = px + (bd.rpb + kWin - 1) * W;

    const float* tp = tru + ((img / S) * (int64_t)H + r0) * W * C + c;
    const float* rp = res + (img * (int64_t)H + r0) * W * C + c;
    const int nload = (rend - r0) * W, nown = (own_end - r0) * W;
    double se = 0.0;
    for (int e = tid; e < nload; e += kBlock) {
        float a = tp[(int64_t)e * C], b = rp[(int64_t)e * C];
        if (clip) {
            a = clip01(a);
            b = clip01(b);
        }
        px[e] = a;
        py[e] = b;
        if (e < nown) {
            const double d = (double)a - (double)b;
            se = se + d * d;
        }
    }
    __syncthreads();

    const int seg = tid / W, x = tid - seg * W;
    const bool lane_on = seg < bd.nseg;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0, acc = 0.0;
    for (int i = 0; i < bd.rps; ++i) {
        const int lr = seg * bd.rps + i;                             // the window row, counted from r0
        const bool on = lane_on && lr < r1 - r0;
        if (on) {
            if (i == 0) {
                sx = sy = sxx = syy = sxy = 0.0;
                for (int k = 0; k < kWin; ++k) {
                    const double a = px[(lr + k) * W + x], b = py[(lr + k) * W + x];
                    sx = sx + a;
                    sy = sy + b;
                    sxx = sxx + a * a;
                    syy = syy + b * b;
                    sxy = sxy + a * b;
                }
            } else {
                const double a = px[(lr + kWin - 1) * W + x], b = py[(lr + kWin - 1) * W + x];
                const double p = px[(lr - 1) * W + x], q = py[(lr - 1) * W + x];
                sx = (sx + a) - p;
                sy = (sy + b) - q;
                sxx = (sxx + a * a) - p * p;
                syy = (syy + b * b) - q * q;
                sxy = (sxy + a * b) - p * q;
            }
            cs[0 * ncs + tid] = sx;
            cs[1 * ncs + tid] = sy;
            cs[2 * ncs + tid] = sxx;
            cs[3 * ncs + tid] = syy;
            cs[4 * ncs + tid] = sxy;
        }
        __syncthreads();
        if (on && x < wout) {
            double w[5];
            for (int q = 0; q < 5; ++q) {
                double s = cs[q * ncs + tid];
                for (int k = 1; k < kWin; ++k) s = s + cs[q * ncs + tid + k];
                w[q] = s;
            }
            const double np = (double)(kWin * kWin), cov_norm = np / (np - 1.0);
            const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
            const double ux = w[0] / np, uy = w[1] / np;
            const double vx = cov_norm * (w[2] / np - ux * ux);
            const double vy = cov_norm * (w[3] / np - uy * uy);
            const double vxy = cov_norm * (w[4] / np - ux * uy);
            const double a1 = 2.0 * (ux * uy) + C1, a2 = 2.0 * vxy + C2;
            const double b1 = (ux * ux + uy * uy) + C1, b2 = (vx + vy) + C2;
            acc = acc + (a1 * a2) / (b1 * b2);
        }
        __syncthreads();
    }
    // the trees reuse cs: ncs = (256 / W) * W >= 129 for every W <= 256, so cs has at least 645 doubles
    cs[tid] = acc;
    tree256(cs);
    const double ssum = cs[0];
    __syncthreads();
    cs[tid] = se;
    tree256(cs);
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = ssum;
        part[2 * (int64_t)blockIdx.x + 1] = cs[0];
    }
}

__global__ void __launch_bounds__(kBlock) k_psnr_ssim_finish(const double* __restrict__ part, int64_t GS, int H, int W, int C,
                                                             int nb, double* __restrict__ psnr, double* __restrict__ ssim) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= GS) return;
    const double nwin = (double)(H - (kWin - 1)) * (double)(W - (kWin - 1));
    double se = 0.0, sc = 0.0;
    for (int c = 0; c < C; ++c) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) {
            const double* p = part + 2 * ((i * C + c) * nb + b);
            s = s + p[0];
            se = se + p[1];
        }
        sc = sc + s / nwin;
    }
    ssim[i] = sc / (double)C;
    const double mse = se / ((double)H * (double)W * (double)C);
    psnr[i] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
}

// ---- chain autocorrelation ----

__global__ void __launch_bounds__(kBlock) k_autocorr(const float* __restrict__ x, int S, int D, int L,
                                                     double* __restrict__ ac) {
    const int d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= D) return;
    const int64_t m = blockIdx.y;
    const float* col = x + m * (int64_t)S * D + d;
    double* out = ac + m * (int64_t)L * D + d;
    const uint32_t first = __float_as_uint(col[0]);
    bool constant = true;
    double sum = 0.0;
    for (int t = 0; t < S; ++t) {
        const float v = col[(int64_t)t * D];
        constant = constant && (__float_as_uint(v) == first);
        sum = sum + (double)v;
    }
    if (constant) {                                                  // the stated rule: NaN at every lag
        for (int k = 0; k < L; ++k) out[(int64_t)k * D] = __builtin_nan("");
        return;
    }
    const double mean = sum / (double)S;
    double var = 0.0;
    for (int t = 0; t < S; ++t) {
        const double cv = (double)col[(int64_t)t * D] - mean;
        var = var + cv * cv;
    }
    var = var / (double)S;
    for (int k = 0; k < L; ++k) {
        double s = 0.0;
        for (int t = 0; t < S - k; ++t) {
            const double a = (double)col[(int64_t)t * D] - mean, b = (double)col[(int64_t)(t + k) * D] - mean;
            s = s + a * b;
        }
        out[(int64_t)k * D] = (s / (double)(S - k)) / var;
    }
}

__global__ void __launch_bounds__(kBlock) k_autocorr_best(const double* __restrict__ ac, int D, double* __restrict__ best) {
    __shared__ double mn[kBlock];
    __shared__ int any[kBlock];
    const int tid = threadIdx.x;
    const double* row = ac + (int64_t)blockIdx.x * D;                // blockIdx.x = chain * L + lag
    double lo = (double)INFINITY;
    int seen = 0;
    for (int d = tid; d < D; d += kBlock) {
        const double v = row[d];
        if (v == v) {
            const double p = v > 0.0 ? v : 0.0;
            lo = p < lo ? p : lo;
            seen = 1;
        }
    }
    mn[tid] = lo;
    any[tid] = seen;
    for (int s = kBlock / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            mn[tid] = mn[tid + s] < mn[tid] ? mn[tid + s] : mn[tid];
            any[tid] = any[tid] | any[tid + s];
        }
    }
    if (tid == 0) best[blockIdx.x] = any[0] ? mn[0] : __builtin_nan("");
}

}  // namespace

}  // namespace fbsmi

using namespace fbsmi;

extern "C" {

size_t fbsmi_img_psnr_ssim_workspace_bytes(int64_t GS, int32_t H, int32_t W, int32_t C) {
    if (GS < 1 || H < kWin || W < kWin || H > 256 || W > 256 || C < 1 || C > 4) return 0;
    return (size_t)GS * (size_t)C * (size_t)bands_for(H, W).nb * 2 * sizeof(double);
}

int fbsmi_img_psnr_ssim_batched(const float* true_imgs, const float* restored, int64_t G, int64_t S, int32_t H, int32_t W,
                                int32_t C, int clip, double* psnr, double* ssim, void* ws, void* stream) {
    FBSMI_NEED(true_imgs && restored && psnr && ssim && ws, "img_psnr_ssim_batched: null pointer");
    FBSMI_NEED(G >= 1 && S >= 1, "img_psnr_ssim_batched: G and S must be at least 1");
    FBSMI_NEED(clip == 0 || clip == 1, "img_psnr_ssim_batched: clip must be 0 or 1");
    if (H < kWin || W < kWin || H > 256 || W > 256 || C < 1 || C > 4)
        return fail(FBSMI_ERR_UNSUPPORTED, "img_psnr_ssim_batched: needs 7 <= H, W <= 256 and 1 <= C <= 4");
    FBSMI_NEED(S <= kMaxGrid && G <= kMaxGrid / S, "img_psnr_ssim_batched: too many images for one grid");
    const int64_t GS = G * S;
    const Bands bd = bands_for(H, W);
    FBSMI_NEED(GS <= kMaxGrid / ((int64_t)C * bd.nb), "img_psnr_ssim_batched: too many images for one grid");
    const size_t lds = (size_t)5 * bd.nseg * W * sizeof(double) + (size_t)2 * (bd.rpb + kWin - 1) * W * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    k_psnr_ssim_band<<<(unsigned)(GS * C * bd.nb), kBlock, lds, st>>>(true_imgs, restored, (int)S, H, W, C, clip, bd,
                                                                     (double*)ws);
    FBSMI_LAUNCH_CHECK();
    k_psnr_ssim_finish<<<(unsigned)((GS + kBlock - 1) / kBlock), kBlock, 0, st>>>((const double*)ws, GS, H, W, C, bd.nb, psnr,
                                                                                  ssim);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

int fbsmi_chain_autocorr_batched(const float* chains, int64_t M, int64_t S, int64_t D, int64_t L, double* ac, double* best,
                                 void* stream) {
    FBSMI_NEED(chains && ac && best, "chain_autocorr_batched: null pointer");
    FBSMI_NEED(M >= 1 && S >= 1 && D >= 1, "chain_autocorr_batched: M, S and D must be at least 1");
    FBSMI_NEED(L >= 1 && L <= S, "chain_autocorr_batched: needs 1 <= L <= S");
    if (M > 65535 || S > (1 << 20) || D > (1 << 24))
        return fail(FBSMI_ERR_UNSUPPORTED, "chain_autocorr_batched: needs M <= 65535, S <= 2^20 and D <= 2^24");
    FBSMI_NEED(M * L <= kMaxGrid, "chain_autocorr_batched: too many (chain, lag) pairs for one grid");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((D + kBlock - 1) / kBlock), (unsigned)M);
    k_autocorr<<<grid, kBlock, 0, st>>>(chains, (int)S, (int)D, (int)L, ac);
    FBSMI_LAUNCH_CHECK();
    k_autocorr_best<<<(unsigned)(M * L), kBlock, 0, st>>>(ac, (int)D, best);
    FBSMI_LAUNCH_CHECK();
    return FBSMI_OK;
}

}  // extern "C"
