/*
 * fbsmi.h -- C ABI of libfbsmi, the MI355X (gfx950) engine for the particle-Gibbs / CSMC / pMCMC
 * hot path of zgbkdlm/fbs.
 *
 * The reference has no FFI: its boundary is the Python API of fbs.samplers / fbs.sdes on JAX
 * arrays.  Each entry point below names the reference function(s) whose
 * device work it performs; fbs_amd/ (Python, ctypes) keeps the reference's names and argument
 * orders on top of it, and INTEGRATION.md shows the binding a maintainer of the reference would
 * add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr()) unless
 *     the parameter is documented "host";
 *   - `stream` is a hipStream_t (NULL = default stream); all work is stream-ordered, nothing
 *     synchronises, nothing allocates: scratch comes from the caller's workspace `ws`
 *     (fbsmi_workspace_bytes);
 *   - PRNG keys are JAX threefry keys, two uint32 passed by value as (k0, k1);
 *   - return value 0 = OK, negative = error (fbsmi_last_error() gives the text); no exceptions
 *     cross the ABI; calls are re-entrant across streams as long as workspaces differ;
 *   - float data is float32, indices int32, row-major.
 */
#ifndef FBSMI_H
#define FBSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FBSMI_ABI_VERSION 1

#define FBSMI_OK 0
#define FBSMI_ERR_ARG (-1)
#define FBSMI_ERR_HIP (-2)
#define FBSMI_ERR_UNSUPPORTED (-3)

int fbsmi_abi_version(void);
const char* fbsmi_last_error(void);

/* ---- PRNG (jax.random.*; call sites listed in SURVEY.md Appendix A) ------------------------- */
/* jax.random.split(key, num) on the HOST (pure integer work; out is a host array of num*2). */
void fbsmi_key_split(uint32_t k0, uint32_t k1, int num, uint32_t* out_host);
int fbsmi_random_bits(uint32_t k0, uint32_t k1, int64_t n, uint32_t* out, void* stream);
int fbsmi_uniform(uint32_t k0, uint32_t k1, int64_t n, float* out, void* stream);
int fbsmi_normal(uint32_t k0, uint32_t k1, int64_t n, float* out, void* stream);
int fbsmi_randint(uint32_t k0, uint32_t k1, int64_t n, int32_t lo, int32_t hi, int32_t* out, void* stream);
/* Elements [start, start+count) of the flat draw of n_total elements (mode 0 bits, 1 uniform,
 * 2 normal): the slice a rank of a sharded particle ensemble owns, identical to the unsharded draw. */
int fbsmi_random_range(int mode, uint32_t k0, uint32_t k1, int64_t n_total, int64_t start, int64_t count, void* out,
                       void* stream);

/* ---- numeric specification probes (include/fbsmi_math.h evaluated on the device) ------------
 * op: 0 exp, 1 log, 2 log1p, 3 erfinv, 4 sqrt, 5 x/y, 6 bits->normal (x reinterpreted as uint32), 7 the same
 * through the kernels' branch-free device form (must equal 6 bit for bit on every input), 8 x/y through the kernels'
 * reciprocal-and-correction form (must equal 5 bit for bit). */
int fbsmi_math_map(int op, const float* x, const float* y, int64_t n, float* out, void* stream);

/* ---- tree reductions / scans -------------------------------------------------------------- */
size_t fbsmi_workspace_bytes(int64_t n);
/* jnp.cumsum (associative_scan order); out may alias x */
int fbsmi_cumsum(const float* x, int64_t n, float* out, void* ws, void* stream);
/* root of the pairwise tree over x (zero padded) -> out[0] */
int fbsmi_sum(const float* x, int64_t n, float* out, void* ws, void* stream);
/* jax.scipy.special.logsumexp -> out[0] */
int fbsmi_logsumexp(const float* x, int64_t n, float* out, void* ws, void* stream);
/* fbs/samplers/csmc/csmc.py:273-292 normalise: out = lw - logsumexp(lw) (exp'd unless log_space);
 * out may alias lw; out_lse (nullable) receives the logsumexp. */
int fbsmi_normalise(const float* lw, int64_t n, int log_space, float* out, float* out_lse, void* ws, void* stream);
/* The same with the two diagnostics a sharded / monitored run reports per step (SURVEY.md 8b `out_ess`; the reference
 * computes neither): out_lse (nullable) = logsumexp(lw), the increment of the log normalising constant when lw are the
 * unnormalised log-weights of a step (csmc.py:146, smc.py:145-146 `c`); out_ess (nullable) = 1 / sum_i w_i^2 with
 * w_i = exp(lw_i - lse) in float32, the sum being the root of the pairwise tree over the index bits. */
int fbsmi_normalise_ess(const float* lw, int64_t n, int log_space, float* out, float* out_lse, float* out_ess, void* ws,
                        void* stream);
/* jnp.searchsorted(a, q, side='left') for m queries */
int fbsmi_searchsorted(const float* a, int32_t n, const float* q, int64_t m, int32_t* out, void* stream);

/* ---- resamplers ---------------------------------------------------------------------------- */
/* fbs/samplers/resampling.py: kind 0 stratified :58, 1 systematic :54, 2 multinomial :62,
 * 3 killing :71.  Reference signature f(weights, key). */
int fbsmi_resample(int kind, const float* w, uint32_t k0, uint32_t k1, int32_t n, int32_t* idx, void* ws,
                   void* stream);
/* fbs/samplers/csmc/resamplings.py: kind 0 multinomial :10, 1 killing :40, 2 systematic :91
 * (conditional systematic is NotImplementedError in the reference -> FBSMI_ERR_UNSUPPORTED).
 * Reference signature f(key, weights, i, j, conditional). */
int fbsmi_cond_resample(int kind, uint32_t k0, uint32_t k1, const float* w, int32_t i, int32_t j, int conditional,
                        int32_t n, int32_t* idx, void* ws, void* stream);
/* jax.random.choice(key, n, (), p=w): csmc.py:295-297 barker_move, smc.py:104 -> out[0] */
int fbsmi_categorical(uint32_t k0, uint32_t k1, const float* w, int32_t n, int32_t* out, void* ws, void* stream);
/* fbs/samplers/gibbs.py:171-214 force_move -> out_i[0], out_alpha[0] (out_alpha nullable) */
int fbsmi_force_move(uint32_t k0, uint32_t k1, const float* w, int32_t k, int32_t n, int32_t* out_i,
                     float* out_alpha, void* ws, void* stream);

/* ---- data movement ------------------------------------------------------------------------- */
/* jnp.take(src, idx, axis=0): dst[r, :] = src[idx[r], :], rows of d floats (csmc.py:140) */
int fbsmi_gather_rows(const float* src, const int32_t* idx, int64_t n, int64_t d, float* dst, void* stream);
/* x.at[row].set(v): dst[row, :] = src[:]  (csmc.py:143,152) */
int fbsmi_set_row(float* dst, int64_t row, const float* src, int64_t d, void* stream);
/* csmc.py:262-267 ancestor back-trace: Bs[T] = B_T[0]; Bs[k-1] = As[k-1, Bs[k]]; As is (T, n) */
int fbsmi_backtrace(const int32_t* As, int32_t T, int32_t n, const int32_t* B_T, int32_t* Bs, void* stream);

/* ---- single-trajectory SDE paths ------------------------------------------------------------
 * out (T+1, D): out[0] = x0, out[k+1] = F[k]*out[k] + S[k]*xi[k]  -- the exact forward noising
 * transition of simulate_cond_forward(keep_path=True), fbs/sdes/linear.py:190-221; xi (T, D).  Any D >= 1 is supported
 * (the launch is capped and strides over the coordinates); T = 0 writes out[0] only. */
int fbsmi_linear_path(const float* F, const float* S, const float* x0, const float* xi, int32_t T, int64_t D,
                      float* out, void* stream);
/* Euler-Maruyama with nsub sub-steps per interval for a drift affine in x:
 *   x += (A[r] x + B[r] target) ddt[k] + S[r] sqrt(ddt[k]) xi,  r = k*nsub + j,
 * xi = normal(keys[k], (nsub, D)) (fbs/sdes/simulators.py:53-106).  With the Doob bridge drift of a
 * scalar linear SDE this is doob_bridge_simulator (simulators.py:126-160), the bridge_sampler of
 * fbs/samplers/gibbs.py:17-20.  keys (T,2) uint32 device; out (T+1, D).  Any D >= 1 is supported (the launch is capped
 * and strides over the coordinates). */
int fbsmi_affine_em_path(const uint32_t* keys, const float* A, const float* B, const float* S, const float* ddt,
                         const float* target, const float* x0, int32_t T, int32_t nsub, int64_t D, int replace_last,
                         float* out, void* stream);

/* Euler-Maruyama with nsub sub-steps per interval for a time-dependent MATRIX-affine drift -- euler_maruyama
 * (fbs/sdes/simulators.py:53-106) of the Gaussian Schrodinger bridge's forward drift (experiments/sb/gibbs.py:137-139,
 * fbs/sdes/linear.py:397-457).  Numeric specification:
 *   interval k of a grid ts (T+1 points): h64 = |ts[k+1] - ts[k]| / nsub (float64), ddt[k] = float32(h64), sub-step
 *   times tau_{k,j} = linspace(ts[k], ts[k+1] - h64, nsub)[j];
 *   sub-step r = k*nsub + j has float32 tables built in float64 on the host and rounded once:
 *     M[r] (D x D, row-major), c[r] (D), s[r] = float32(dispersion(tau_{k,j}) * sqrt(h64));
 *   noise xi_k = normal(split(key, T)[k], (nsub, D)), row j for sub-step j (euler_maruyama's key schedule);
 *   f_i  = c[r][i] + sum_c M[r][i][c] * x_c      -- one fbsmi_fmaf chain started at c[r][i], c = 0 .. D-1
 *   x_i <- (x_i + f_i * ddt[k]) + s[r] * xi_k[j][i]   -- separate float32 operations, nothing else fused
 *   out[0] = x0, out[k+1] = x after interval k.
 * Tables are device arrays covering T*nsub sub-steps of dimension D. */
typedef struct fbsmi_em_forward {
    int32_t nsub;
    const float* M;    /* [T*nsub][D][D] */
    const float* c;    /* [T*nsub][D] */
    const float* ddt;  /* [T] */
    const float* s;    /* [T*nsub] */
} fbsmi_em_forward;

/* One path, one workgroup: keys (T,2) uint32 = split(key, T), x0 (D), out (T+1, D); D <= 256. */
int fbsmi_lg_em_path(const uint32_t* keys, const fbsmi_em_forward* f, const float* x0, int32_t T, int64_t D, float* out,
                     void* stream);

/* One Euler-Maruyama sub-step for a drift tensor the caller evaluated (a score network, any closure):
 *   out[e] = (x[e] + drift[e] * ddt) + c * xi[offset + e],  xi = jax.random.normal(key, (n_total,)) drawn in the kernel,
 * the loop body of euler_maruyama (fbs/sdes/simulators.py:94-99) with c = dispersion(t) * sqrt(ddt); sub-step j of an interval
 * is offset = j * n of the (integration_nsteps, *x.shape) draw of simulators.py:91.  out may alias x. */
int fbsmi_em_update(const float* x, const float* drift, float ddt, float c, uint32_t k0, uint32_t k1, int64_t n_total,
                    int64_t offset, int64_t n, float* out, void* stream);

/* ---- fused linear-Gaussian sampler ------------------------------------
 * The reverse drift of a scalar-coefficient linear SDE under a Gaussian prior is affine,
 * f(z, t_k) = G_k z + g_k; the three closures of experiments/toy/gp_gibbs.py:120-135 then need no
 * Python in the loop.  Tables (device, float32), T = number of steps, D = du + dv:
 *   G [T][D][D], g [T][D], sd [T] = sqrt(dt)*dispersion, lognorm [T] = log(2 pi sd^2),
 *   F [T], sqQ [T] forward transition ts[k] -> ts[k+1].                                        */
typedef struct fbsmi_lg_model {
    int32_t du, dv, T;
    float dt;
    const float* G;
    const float* g;
    const float* sd;
    const float* lognorm;
    const float* F;
    const float* sqQ;
} fbsmi_lg_model;

/* The three model closures on (n, du) ROW-MAJOR particles for step k (t_prev = ts[k]); sd_k and
 * lognorm_k are the host copies of sd[k], lognorm[k] (the tables themselves live on the device).
 * transition_sampler / likelihood_logpdf / transition_logpdf of experiments/toy/gp_gibbs.py:120-135. */
int fbsmi_lg_transition_sampler(const fbsmi_lg_model* m, int32_t k, float sd_k, float lognorm_k, const float* us_prev,
                                const float* v_prev, uint32_t k0, uint32_t k1, int64_t n, float* us, void* stream);
/* transition_sampler for rows [row0, row0+n) of an ensemble of n_total rows (sharded ensembles):
 * us_prev / us hold only those n rows; the noise is the matching slice of the global draw. */
int fbsmi_lg_transition_sampler_rows(const fbsmi_lg_model* m, int32_t k, float sd_k, float lognorm_k,
                                     const float* us_prev, const float* v_prev, uint32_t k0, uint32_t k1,
                                     int64_t n_total, int64_t row0, int64_t n, float* us, void* stream);
int fbsmi_lg_likelihood_logpdf(const fbsmi_lg_model* m, int32_t k, float sd_k, float lognorm_k, const float* v,
                               const float* us_prev, const float* v_prev, int64_t n, float* lw, void* stream);
int fbsmi_lg_transition_logpdf(const fbsmi_lg_model* m, int32_t k, float sd_k, float lognorm_k, const float* u,
                               const float* us_prev, const float* v_prev, int64_t n, float* lw, void* stream);

typedef struct fbsmi_lg_sweep fbsmi_lg_sweep; /* opaque: device buffers + captured hipGraph */

/* Create the state for gibbs_kernel sweeps (fbs/samplers/gibbs.py:68-168; marg_y=False until
 * fbsmi_lg_sweep_set_bridge switches the handle to marg_y=True) with
 * `nparticles` particles, for `nchains` independent chains batched in every launch -- the
 * reference's jax.vmap over chains (experiments/toy/gp_gibbs.py:25,172-173).  store_path != 0 keeps
 * As / uss / log_wss (needed when explicit_backward == 0).  Allocates device memory (not
 * stream-ordered; call once).  All per-chain arrays below are laid out [nchains][...].
 * A handle owns one launch stream and one set of buffers: calls on the SAME handle must not overlap
 * (drive a handle from one host thread at a time); different handles are independent. */
int fbsmi_lg_sweep_create(const fbsmi_lg_model* model, int32_t nparticles, int explicit_backward,
                          int explicit_final, int store_path, int32_t nchains, fbsmi_lg_sweep** out);
void fbsmi_lg_sweep_destroy(fbsmi_lg_sweep* s);
/* One Gibbs sweep of every chain, everything on the device.  keys (C,2) uint32, x0 (C,du),
 * y0 (dv) shared, bs_star (C,T+1) are device inputs; x0_next (C,du), us_star_next (C,T+1,du),
 * bs_next (C,T+1), acc (C,T+1) bytes are device outputs (nullable; may alias the inputs of the next
 * call).  use_graph != 0 replays a hipGraph captured on the first call. */
int fbsmi_lg_gibbs_sweep(fbsmi_lg_sweep* s, const uint32_t* keys, const float* x0, const float* y0,
                         const int32_t* bs_star, float* x0_next, float* us_star_next, int32_t* bs_next,
                         uint8_t* acc, int use_graph, void* stream);
/* Chain `nsweeps` sweeps with the key schedule of the reference's drivers: per sweep
 * key, subkey = split(key); one chain sweeps with subkey (tests/test_gibbs.py:115-118), a batch of
 * C > 1 chains with split(subkey, C)[c] (experiments/toy/gp_gibbs.py:183-185).  key (2), x0 (C,du),
 * bs_star (C,T+1) are updated in place; x0s (nullable) receives (nsweeps, C, du). */
int fbsmi_lg_gibbs_chain(fbsmi_lg_sweep* s, uint32_t* key, float* x0, const float* y0, int32_t* bs_star,
                         int32_t nsweeps, float* x0s, int use_graph, void* stream);
/* A batch of chains may be driven as several handles ("groups") of fewer chains each, on their own streams: the step
 * kernels of a toy-sized ensemble are latency-bound (~3 us of every launch are its boundaries), so two half-size batches
 * whose launches interleave finish sooner than one full-size batch.  set_group tells a handle which chains of the batch it
 * drives (key schedule split(subkey, nchains_total)[first_chain + c], rows of x0s); call it before the handle's first
 * chain sweep.  chain_groups is fbsmi_lg_gibbs_chain over the handles (which must cover chains 0 .. nchains_total-1 in
 * order): same arguments, same results bit for bit, per-chain arrays laid out for the whole batch. */
int fbsmi_lg_sweep_set_group(fbsmi_lg_sweep* s, int32_t nchains_total, int32_t first_chain);
int fbsmi_lg_gibbs_chain_groups(fbsmi_lg_sweep* const* groups, int32_t ngroups, uint32_t* key, float* x0, const float* y0,
                                int32_t* bs_star, int32_t nsweeps, float* x0s, int use_graph, void* stream);
/* Forward process by Euler-Maruyama: the sweep's two forward paths (key_fwd from (x0, y0) and, with explicit_backward,
 * the fresh reference path from (x0_next, y0)) follow fbsmi_lg_em_path on these tables instead of the exact transition
 * F / sqQ, which the handle then never reads (an SB model passes placeholders).  The CSMC part reads G, g, sd, lognorm as
 * always.  Call once, before the handle's first sweep; the tables must cover the model's T and D = du + dv and outlive the
 * handle.  Allocates the handle's noise workspace (2 * nchains * T * nsub * D floats). */
int fbsmi_lg_sweep_set_em_forward(fbsmi_lg_sweep* s, const fbsmi_em_forward* f);
/* marg_y=True (gibbs.py:17-20,130): every sweep of the handle re-draws the observation path by the Doob bridge of the
 * scalar linear SDE, bridge_sampler = doob_bridge_simulator(key_bridge, sde, y_0, y_T, ts, integration_nsteps = nsub,
 * replace = True).  After the forward path of key_fwd has produced path_y, vs = reverse(bridge), where bridge is exactly
 * what fbsmi_affine_em_path defines with x0 = path_y[0], target = path_y[T], keys split(key_bridge, T), key_bridge =
 * split(key, 3)[2], replace_last = 1; us_star, the CSMC, the forced move and the second forward path are untouched.
 * Numeric specification (fbsmi_affine_em_path's, restated; no contraction, every operation separately rounded), for
 * sub-step j of interval k, r = k * nsub + j, coordinate c, tg = target[c]:
 *   sq = fbsmi_sqrtf(ddt[k]);  drift = A[r] * x + B[r] * tg;  x = (x + drift * ddt[k]) + (S[r] * sq) * xi,
 *   xi = element j * dv + c of normal(split(key_bridge, T)[k], (nsub, dv)).
 * A, B, S: [T * nsub] device float32 (the bridge drift's two scalar coefficients and the dispersion at every sub-step
 * time), ddt: [T].  Call once, before the handle's first sweep.  The tables are read DURING this call only, after a device-wide
 * synchronise (they need not outlive it): the handle keeps its own packed copy and allocates the bridge's noise
 * workspace (nchains * T * nsub * dv floats).  FBSMI_ERR_UNSUPPORTED on a handle with an
 * Euler-Maruyama forward process (such a model has no scalar linear SDE to bridge). */
typedef struct fbsmi_doob_bridge {
    int32_t nsub;
    const float* A;
    const float* B;
    const float* S;
    const float* ddt;
} fbsmi_doob_bridge;
int fbsmi_lg_sweep_set_bridge(fbsmi_lg_sweep* s, const fbsmi_doob_bridge* b);
/* Opt-in per-step diagnostics of the fused engines (the reference computes neither).  For a vector lw of n unnormalised
 * float32 log-weights a diagnostic row is (lse, ess):
 *   lse = the project's logsumexp of lw: the two-level tiled definition of include/fbsmi_math.h, tile fbsmi_tile(n);
 *   ess = 1 / S, S the root of the canonical pairwise tree over w_i * w_i, w_i = fbsmi_expf(lw_i - lse); the division is
 *         float32 and correctly rounded.
 * These are the definitions of fbsmi_normalise_ess: no other numeric convention.  The vectors:
 *   Gibbs sweep (n = nparticles, +1 with explicit_final): T + 1 rows per chain.  Row 0: the initial log-weights before
 *     normalise (explicit_final: the init likelihood, gibbs.py:136-137; else the constant -log n vector, :143-144);
 *     row k = 1..T: the likelihood_logpdf values of step k - 1 (csmc.py:145, before :146).
 *   Filter flow 0 (bootstrap_filter): T rows, row k = log_weights of smc.py:65, its lse the _c of :66.
 *   Filter flow 1 (pmcmc_filter_step): T rows, row k = log_ws of smc.py:144, its lse the _c of :145.
 * fbsmi_lg_sweep_set_diagnostics(s, 1) allocates nchains * (T + 1) * 2 floats and adds the diagnostic launches to the
 * handle's launch list (one graph replay per sweep still; narrow ensembles of one tile then take one launch per step instead
 * of one per sweep).  Call it before the handle's first sweep (FBSMI_ERR_ARG afterwards); it combines with set_bridge,
 * set_em_forward, set_group and fbsmi_lg_gibbs_chain.  The buffer holds the rows of the LAST sweep; view 7 fetches it.
 * A handle without diagnostics launches exactly what it launched before these entry points existed. */
int fbsmi_lg_sweep_set_diagnostics(fbsmi_lg_sweep* s, int enable);
/* Parity views of the last sweep: copies view `which` into dst (device, nullable) and reports its
 * element count.  which: 0 final particles (n,du) row-major, 1 final normalised log-weights (n),
 * 2 As (T,n) int32, 3 uss (T+1,n,du), 4 log_wss (T+1,n) [2-4 only with store_path],
 * 5 us_star (T+1,du) and 6 vs (T+1,dv) of the sweep, 7 the diagnostic rows (T+1,2), [..,0] = lse, [..,1] = ess
 * (FBSMI_ERR_ARG on a handle without diagnostics); each with a leading [nchains] axis; any other
 * `which` is FBSMI_ERR_ARG.  n = nparticles (+1 if explicit_final). */
int fbsmi_lg_sweep_view(fbsmi_lg_sweep* s, int which, void* dst, int64_t* count, void* stream);
/* Fused particle filters for the analytic model, stratified (resampling = 0) or systematic (1)
 * resampling (fbs/samplers/resampling.py:43-59):
 *   flow 0  bootstrap_filter (fbs/samplers/smc.py:9-88); loglik receives the NEGATIVE log-likelihood
 *           estimate; with store_path the filtering path (T+1, n, du) can be fetched (return_last=False);
 *   flow 1  pmcmc_filter_step (smc.py:115-158); loglik receives log_ell.
 * keys (C,2), vs (C,T+1,dv) the reversed observation path, u0s (C,n,du) row-major initial particles
 * are device inputs; uT (C,n,du), loglik (C), path (C,T+1,n,du) device outputs (nullable). */
typedef struct fbsmi_lg_filter fbsmi_lg_filter;
int fbsmi_lg_filter_create(const fbsmi_lg_model* model, int32_t nparticles, int flow, int resampling, int store_path,
                           int32_t nchains, fbsmi_lg_filter** out);
void fbsmi_lg_filter_destroy(fbsmi_lg_filter* f);
int fbsmi_lg_filter_run(fbsmi_lg_filter* f, const uint32_t* keys, const float* vs, const float* u0s, float* uT,
                        float* loglik, float* path, int use_graph, void* stream);
/* The diagnostics of fbsmi_lg_sweep_set_diagnostics (defined there) for a filter handle: call set_diagnostics before the
 * handle's first run; fbsmi_lg_filter_diag copies the (nchains, T, 2) rows of the LAST run into dst (device, nullable) and
 * reports their element count; FBSMI_ERR_ARG on a handle without diagnostics. */
int fbsmi_lg_filter_set_diagnostics(fbsmi_lg_filter* f, int enable);
int fbsmi_lg_filter_diag(fbsmi_lg_filter* f, void* dst, int64_t* count, void* stream);

/* Fused particle-marginal Metropolis-Hastings for the analytic model: pmcmc_kernel (fbs/samplers/smc.py:171-258, with
 * delta = None or the pCN proposal of smc.py:161-168) for `nchains` chains in every launch, inside the loop of
 * experiments/toy/gp_pmcmc.py:163-179.  One iteration is three launches round the flow-1 filter above (keys + proposal
 * path + reversal; initial particles; accept), captured with it in one hipGraph; nothing returns to the host between
 * iterations.  The tables are device arrays built ONCE on the host in float64 from (m_ref, cov_ref) = forward_m_cov(T)
 * (gp_gibbs.py:84-86): m_u = m_ref[:du], m_v = m_ref[du:], gain = cov_ref[:du, du:] inv(cov_ref[du:, du:]),
 * chol = float32(cholesky(cov_ref[:du, :du] - gain cov_ref[du:, :du])) (lower), mean_coef[k] = float32(sde.mean(ts[k],
 * ts[0], 1)).  They must outlive the handle.
 * Numeric specification (no contraction anywhere; every operation separately rounded):
 *   forward path   r[0] = y0, r[k+1] = F[k] * r[k] + sqQ[k] * xi[k], xi = normal(key, (T, dv))  (fbsmi_linear_path);
 *   pCN            mean[k] = mean_coef[k] * y0;  p = ys[k] + c0 * (r0[k] - mean[k]);
 *                  prop_ys[k] = (beta * p + one_minus_beta * mean[k]) + c1 * (r1[k] - mean[k]),  float32, where r0, r1
 *                  are the paths of split(key_prop, 2) and c0 = float32(sqrt(delta / 2)), beta = float32(2 / (2 + delta)),
 *                  one_minus_beta = float32(1 - 2 / (2 + delta)), c1 = float32(sqrt(1 - 2 / (2 + delta)));
 *   ref_sampler    (gp_pmcmc.py:130-133) with yT = prop_ys[T]:
 *                  m_[j] = float32( m_u[j] + s_j ), s_j = 0, then s_j = s_j + gain[j][c] * (double(yT[c]) - m_v[c]) for
 *                  c = 0 .. dv-1, float64;  z = normal(key_u0, (n, du));
 *                  acc = z[i][0] * chol[0][j], then acc = acc + z[i][c] * chol[c][j] for c = 1 .. du-1, float32;
 *                  u0[i][j] = m_[j] + acc;
 *   accept         log_acc = minimum(0, prop_log_ell - log_ell); accepted = fbsmi_logf(uniform(key_mh, ())) < log_acc;
 *                  acceptance_prob = fbsmi_expf(log_acc).
 * Keys: key_prop, key_u0, key_filter, key_mh = split(key, 4) (smc.py:231). */
typedef struct fbsmi_lg_pmcmc_tables {
    const double* m_u;       /* (du) */
    const double* m_v;       /* (dv) */
    const double* gain;      /* (du, dv) */
    const float* chol;       /* (du, du) lower factor */
    const float* mean_coef;  /* (T+1), pCN only (nullable) */
    float c0, beta, one_minus_beta, c1; /* pCN constants */
    int32_t use_pcn;         /* 0: independent proposals (delta = None) */
    int32_t which_u;         /* the particle of the filter's output that is proposed (smc.py:244) */
} fbsmi_lg_pmcmc_tables;
typedef struct fbsmi_lg_pmcmc fbsmi_lg_pmcmc; /* opaque: a flow-1 filter, the chain state and the captured graphs */
/* resampling 0 stratified | 1 systematic.  FBSMI_ERR_UNSUPPORTED for what fbsmi_lg_filter_create does not take and for a
 * model without an exact forward transition (Euler-Maruyama forward process: F and sqQ are all-zero placeholders). */
int fbsmi_lg_pmcmc_create(const fbsmi_lg_model* model, const fbsmi_lg_pmcmc_tables* tables, int32_t nparticles,
                          int resampling, int32_t nchains, fbsmi_lg_pmcmc** out);
void fbsmi_lg_pmcmc_destroy(fbsmi_lg_pmcmc* h);
/* One iteration with explicit per-chain keys (C,2).  The state uT (C,du), log_ell (C), ys (C,T+1,dv) is updated in
 * place; y0 (dv) is shared by the chains.  Nullable outputs: acc_prob (C), accepted (C) bytes, prop_log_ell (C). */
int fbsmi_lg_pmcmc_step(fbsmi_lg_pmcmc* h, const uint32_t* keys, float* uT, float* log_ell, float* ys, const float* y0,
                        float* acc_prob, uint8_t* accepted, float* prop_log_ell, int use_graph, void* stream);
/* nsamples iterations with the driver's key schedule (gp_pmcmc.py:171-172): per iteration key, subkey = split(key) and
 * chain c takes split(subkey, C)[c], for every C >= 1; key (2) is advanced in place, on the device.  samples
 * (nsamples, C, du) receives the state uT after every iteration, acc_prob / accepted (bytes) / prop_log_ell / log_ells
 * (nsamples, C) the fields of MCMCState (fbs/samplers/common.py; log_ell is the state's value BEFORE the decision,
 * smc.py:254); each nullable. */
int fbsmi_lg_pmcmc_chain(fbsmi_lg_pmcmc* h, uint32_t* key, float* uT, float* log_ell, float* ys, const float* y0,
                         int32_t nsamples, float* samples, float* acc_prob, uint8_t* accepted, float* prop_log_ell,
                         float* log_ells, int use_graph, void* stream);

/* Fused bootstrap-filter conditional sampler for the analytic model: conditional_sampler of
 * experiments/toy/gp_filter.py:134-142 for `nsamples` = B independent samples in every launch.  A call is the front
 * launch (keys + forward observation path + reversal + conditional mean), the initial particles, the flow-0 filter's own
 * launch list with nchains = B, and one tail launch, captured in one hipGraph; nothing returns to the host inside a call.
 * Of the tables only m_u, m_v, gain and chol are read (the rest may be zero); they must outlive the handle.
 * Numeric specification (no contraction anywhere; every operation separately rounded), sample b with key = keys[b]:
 *   keys           key_fwd, key_bwd, key_bf = split(key, 3) (gp_filter.py:135; key_bwd is unused, as in the reference);
 *                  key_init = split(key_bf, 2)[0] (smc.py:77);
 *   forward path   r[0] = y0, r[k+1] = F[k] * r[k] + sqQ[k] * xi[k], xi = normal(key_fwd, (T, dv))  (fbsmi_linear_path);
 *                  vs[k] = r[T - k];
 *   ref_sampler    u0s = ref_sampler(key_init, vs[0], n), exactly the ref_sampler block of fbsmi_lg_pmcmc above
 *                  (float64 conditional mean in ascending c; float32 acc over chol in ascending c; u0 = m_ + acc);
 *   filter         fbsmi_lg_filter_run, flow 0, with key key_bf (it derives split(key_bf, 2)[1] itself), vs, u0s and
 *                  the handle's resampling;
 *   outputs        samples[b] = uT[b][0] (the first particle); nell[b] = the filter's negative log-likelihood estimate.
 * resampling 0 stratified | 1 systematic.  FBSMI_ERR_UNSUPPORTED for what fbsmi_lg_filter_create(..., nchains = nsamples)
 * does not take, for nsamples > 65535 and for a model without an exact forward transition (F and sqQ all-zero
 * placeholders); FBSMI_ERR_ARG for null tables. */
typedef struct fbsmi_lg_fsamp fbsmi_lg_fsamp; /* opaque: a flow-0 filter of B chains, the call's keys and outputs, the graph */
int fbsmi_lg_fsamp_create(const fbsmi_lg_model* model, const fbsmi_lg_pmcmc_tables* tables, int32_t nparticles,
                          int resampling, int32_t nsamples, fbsmi_lg_fsamp** out);
void fbsmi_lg_fsamp_destroy(fbsmi_lg_fsamp* h);
/* The same engine for a model whose forward process is Euler-Maruyama (the Gaussian Schrodinger bridge): conditional_sampler
 * of experiments/sb/filter.py:149-161 with fwd_ys_sampler of :137-148, both --x0 modes, for `nsamples` = B independent
 * samples in every launch.  Only the front launch differs: the observation path is the y half of fbsmi_lg_em_path's joint
 * (x, y) path from a drawn x0; the initial particles, the flow-0 filter and the tail are those of fbsmi_lg_fsamp_create,
 * and fbsmi_lg_fsamp_run / _view / _destroy serve the handle.  `fwd` covers the model's T and D = du + dv; x0_mean (du)
 * and x0_chol (du, du), the LOWER factor, are device float32 arrays, both null for x0 ~ N(0, I) ('heuristic') or both set
 * ('proper').  fwd's tables, the tables' m_u, m_v, gain, chol and the prior must outlive the handle.
 * Numeric specification (no contraction anywhere; every operation separately rounded), sample b with key = keys[b]:
 *   keys           key_fwd, key_bwd, key_bf = split(key, 3) (sb/filter.py:153; key_bwd is unused, as in the reference);
 *                  key_x0, key_em = split(key_fwd, 2) (:138);  key_init = split(key_bf, 2)[0] (smc.py:77);
 *   x0             z = normal(key_x0, (du,));  heuristic: x0 = z;  proper: acc = z[0] * x0_chol[0][j], then
 *                  acc = acc + z[c] * x0_chol[c][j] for c = 1 .. du-1, float32;  x0[j] = x0_mean[j] + acc
 *                  (mean + z @ chol in ref_sampler's order);
 *   forward path   out = exactly the fbsmi_em_forward block above from concat(x0, y0) with key key_em: interval k draws
 *                  normal(split(key_em, T)[k], (nsub, D)), element j * D + i for sub-step j, coordinate i;
 *                  vs[T] = y0, vs[T - 1 - k][c] = out[k + 1][du + c]  (the x half is never stored);
 *   ref_sampler    u0s = ref_sampler(key_init, vs[0], n), exactly the ref_sampler block of fbsmi_lg_pmcmc above;
 *   filter, outputs   as fbsmi_lg_fsamp_create.
 * FBSMI_ERR_ARG for a null fwd or tables (or a null array in either), fwd->nsub < 1, and exactly one of x0_mean / x0_chol
 * null; FBSMI_ERR_UNSUPPORTED for du + dv > 256, nsamples > 65535 and what fbsmi_lg_filter_create(..., nchains =
 * nsamples) does not take.  (fbsmi_lg_fsamp_create keeps refusing such a model.) */
int fbsmi_lg_fsamp_create_em(const fbsmi_lg_model* model, const fbsmi_em_forward* fwd,
                             const fbsmi_lg_pmcmc_tables* tables, const float* x0_mean, const float* x0_chol,
                             int32_t nparticles, int resampling, int32_t nsamples, fbsmi_lg_fsamp** out);
/* keys (B,2) and y0 (dv) are device inputs, samples (B,du) and nell (B) (nullable) device outputs. */
int fbsmi_lg_fsamp_run(fbsmi_lg_fsamp* h, const uint32_t* keys, const float* y0, float* samples, float* nell,
                       int use_graph, void* stream);
/* Parity views of the last run: copies view `which` into dst (device, nullable) and reports its element count.
 * which: 0 vs (B,T+1,dv), 1 u0s (B,n,du), 2 uT (B,n,du); any other `which` is FBSMI_ERR_ARG. */
int fbsmi_lg_fsamp_view(fbsmi_lg_fsamp* h, int which, void* dst, int64_t* count, void* stream);

/* ---- fused backward simulation for the analytic model, batched over chains -----------------------
 * mode 0  bootstrap_backward_smoother (fbs/samplers/smc.py:91-112) on a stored filtering path;
 * mode 1  backward_sampling_pass (fbs/samplers/csmc/csmc.py:167-227), the backward pass of csmc_kernel(backward=True),
 *         on the stored particles and normalised log-weights of a CSMC forward pass.
 * nslots = n, the rows of a time slice (particles; particles + 1 for a CSMC forward pass).  The handle reads only
 * G, g, sd, lognorm and dt of the model (F and sqQ may be placeholders).  Supported: 1 <= n <= 131072 (one-item
 * logsumexp tiles, fbsmi_tile_items(n) == 1) and max(du, dv) <= 128; anything else is FBSMI_ERR_UNSUPPORTED.
 * Numeric specification (no contraction anywhere; every operation separately rounded):
 *   tlp(t, x, i)   acc_r = g[t][r], then acc_r = fbsmi_fmaf(G[t][r][c], z[c], acc_r) for c ascending over
 *                  z = (path[t][i], vs[t]);  mean_r = path[t][i][r] + acc_r * dt;
 *                  lp_r = (lognorm[t] + ((x_r - mean_r) * (x_r - mean_r)) / (sd[t] * sd[t])) / -2;
 *                  tlp = lp_0, then + lp_r for r = 1 .. du-1                 (transition_logpdf, gp_gibbs.py:124-129);
 *   lse(x)         the two-level logsumexp of fbsmi_math.h;
 *   cat(key, w)    c = cumsum(w) in the canonical tree order (fbsmi_cumsum); r = c[n-1] * (1 - uniform(key, ()));
 *                  the fixed-length bisection of fbsmi_searchsorted on (c, r)                        (fbsmi_categorical);
 *   mode 0         iT = randint(key, (), 0, n) with the PARENT key (smc.py:109); keys = split(split(key, 2)[1], T);
 *                  traj[T] = path[T][iT]; for s = 0 .. T-1, t = T-1-s: lw_i = tlp(t, traj[t+1], i);
 *                  w_i = fbsmi_expf(lw_i - lse(lw)); traj[t] = path[t][cat(keys[s], w)];
 *   mode 1         keys = split(key, T+1); B_T = cat(keys[T], fbsmi_expf(log_wss[T] - lse(log_wss[T])));
 *                  for s = 0 .. T-1, t = T-1-s: gl_i = tlp(t, traj[t+1], i); x_i = (gl_i - max(gl)) + log_wss[t][i];
 *                  w_i = fbsmi_expf(x_i - lse(x)); B_t = cat(keys[s], w); bs[t] = B_t, traj[t] = path[t][B_t].
 * keys (C,2), vs (C,T+1,dv), path (C,T+1,n,du) row-major, log_wss (C,T+1,n) (mode 1 only) are device inputs; path and
 * log_wss are read in place (never copied) and must stay valid until the call's work on `stream` has finished.
 * traj (C,T+1,du) and bs (C,T+1) (mode 1; nullable) are device outputs.  use_graph != 0 replays one linear hipGraph
 * captured on the handle's first call. */
typedef struct fbsmi_lg_backsim fbsmi_lg_backsim;
int fbsmi_lg_backsim_create(const fbsmi_lg_model* model, int32_t nslots, int mode, int32_t nchains, fbsmi_lg_backsim** out);
void fbsmi_lg_backsim_destroy(fbsmi_lg_backsim* h);
int fbsmi_lg_backsim_run(fbsmi_lg_backsim* h, const uint32_t* keys, const float* vs, const float* path, const float* log_wss,
                         float* traj, int32_t* bs, int use_graph, void* stream);

/* ---- fused twisted SMC for the analytic Gaussian model, batched over runs ------------------------
 * twisted_smc (fbs/samplers/smc.py:261-309) with the closures of experiments/toy/gp_twisted.py:100-129 for a Gaussian
 * prior N(mean, cov) of x and the observation y of x + N(0, obs_var I): the twisting function is a Gaussian density of
 * an affine map of the particle, so its gradient (gp_twisted.py:87-89, jax.grad) is affine and a step is two matrix
 * products and three row-summed Gaussian log-densities.  Tables, one entry per time point j = 0..T of the grid ts
 * (twisted_smc evaluates the closures at ts[0] for the initial twist and at ts[k+1] in step k); with s = ts[T] - ts[j],
 * F, Q = discretise(s, ts[0]), P = inv(F^2 cov + Q I), a = drift(1, s), b = dispersion(s), dt = (ts[T] - ts[0]) / T:
 *   R[j] = -a I - b^2 P,  r[j] = b^2 P (F mean)                     reverse drift rd(u) = R u + r
 *   B    = I + dt R[j]                                               (the denoising estimate is B u + dt r)
 *   C[j] = R[j] - (b^2 / obs_var) B^T B,  c[j] = r[j] + (b^2 / obs_var) B^T (y - dt r[j])
 *                                                                    conditional reverse drift rcd(u) = C u + c
 *   sd[j] = sqrt(dt) b,  lognorm[j] = log(2 pi sd[j]^2),  lognorm_obs = log(2 pi obs_var)
 *   m_ref = F_T mean,  Lt = transpose of the lower Cholesky factor of F_T^2 cov + Q_T I   (F_T, Q_T: j = 0)
 * built in float64 on the host and rounded once to float32 (fbs_amd/lg_twisted.py, lg_twisted_tables).
 *
 * Numeric specification (float32, no contraction; tests/tw_restate.py restates it in numpy):
 *   drift_i(M, m, u): acc = m_i, then acc = fbsmi_fmaf(M[i][c], u[c], acc) for c ascending
 *   nlp(x, loc, s2, ln) = (ln + ((x - loc) * (x - loc)) / s2) / -2;  a row sum is acc = term_0, then acc + term_i, i ascending
 *   twist_j(u) = sum_i nlp(y_i, u_i + drift_i(R[j], r[j], u) * dt, obs_var, lognorm_obs)
 *   init: key_init, key_filter = split(key); keys = split(key_filter, T); z = normal(key_init, (N, d));
 *         x[n][i] = m_ref[i] + acc with acc = z[n][0] * Lt[0][i], then acc + z[n][c] * Lt[c][i];
 *         log_ps = twist_0(x); log_ws = log_ps - logsumexp(log_ps)   (the two-level logsumexp of fbsmi_math.h)
 *   step k (j = k + 1): key_resampling, key_prop = split(keys[k]); inds = resampling(fbsmi_expf(log_ws), key_resampling);
 *         xp = x[inds], lpp = log_ps[inds]; m_i = xp_i + drift_i(C[j], c[j], xp) * dt; x_i = m_i + sd[j] * z_i with
 *         z = normal(key_prop, (N, d)); log_ps = twist_j(x);
 *         tl = sum_i nlp(x_i, xp_i + drift_i(R[j], r[j], xp) * dt, sd[j]^2, lognorm[j]);
 *         pl = sum_i nlp(x_i, m_i, sd[j]^2, lognorm[j])              (from the stored x_i and m_i)
 *         lw = ((tl + log_ps) - pl) - lpp; log_ws = lw - logsumexp(lw)
 *   selection (select != 0): key_filter, key_select = split(key) in front of the run, and after it
 *         jax.random.choice(key_select, N, p = fbsmi_expf(log_ws)) picks the returned row (gp_twisted.py:133-141). */
typedef struct fbsmi_tw_model {
    int32_t d, T;
    float dt;
    const float* R;       /* (T+1, d, d) */
    const float* r;       /* (T+1, d) */
    const float* C;       /* (T+1, d, d) */
    const float* c;       /* (T+1, d) */
    const float* sd;      /* (T+1) */
    const float* lognorm; /* (T+1) */
    const float* m_ref;   /* (d) */
    const float* Lt;      /* (d, d) */
    const float* y;       /* (d) */
    float obs_var, lognorm_obs;
} fbsmi_tw_model;
typedef struct fbsmi_tw fbsmi_tw; /* opaque: device buffers for nruns runs, a stream and the captured graphs */
/* resampling 0 stratified | 1 systematic.  The tables stay the caller's and must outlive the handle.  d outside
 * [1, 128], nparticles outside [1, 131072] or nruns > 65535 (a run is one grid row of every launch):
 * FBSMI_ERR_UNSUPPORTED.  store_ancestors: keep every step's ancestors. */
int fbsmi_tw_create(const fbsmi_tw_model* model, int32_t nparticles, int resampling, int32_t nruns, int store_ancestors,
                    fbsmi_tw** out);
void fbsmi_tw_destroy(fbsmi_tw* h);
/* nruns independent runs, one per key of keys (nruns, 2).  Nullable outputs: xs (nruns, N, d) the final particles,
 * log_ws (nruns, N) their normalised log-weights, samples (nruns, d) the selected rows (select != 0 only). */
int fbsmi_tw_run(fbsmi_tw* h, const uint32_t* keys, int select, float* xs, float* log_ws, float* samples, int use_graph,
                 void* stream);
/* State of the last run, copied to dst (nullable: only *count is set), 4-byte elements: which 0 the ancestors of every
 * step (nruns, T, N) int32 (store_ancestors); of the last step: 1 log_ps, 2 tl, 3 pl (nruns, N), 4 the particles it
 * started from (nruns, N, d), 5 its ancestors (nruns, N) int32. */
int fbsmi_tw_view(fbsmi_tw* h, int which, void* dst, int64_t* count, void* stream);

/* ---- fused, batched conditional score sampler (CSGM) for the analytic Gaussian model --------------
 * The `csgm` method of experiments/toy/gp_csgm.py (Song et al., 2021) for a Gaussian prior N(mean, cov) of x and the
 * observation y of x + N(0, obs_var I): the marginal score and the score of p(y | u_t) are both Gaussian, so the reverse
 * drift is affine, f(u) = A[k] u + cvec[k] (gp_csgm.py:80-94 takes the second score with jax.grad).  Tables, one entry
 * per step k = 0..T-1 of the grid ts; with s = ts[T] - ts[k], F, Q = discretise(s, ts[0]), a = drift(1, s),
 * b = dispersion(s), Sx = F^2 cov + Q I, M = F cov inv(Sx), cond_cov = cov + obs_var I - M (F cov),
 * Gm = M^T inv(cond_cov):
 *   A[k]    = -a I + b^2 (-inv(Sx) - Gm M)
 *   cvec[k] = b^2 (inv(Sx) F mean + Gm (y - mean + M F mean))
 *   ddt[k]  = float32(|ts[k+1] - ts[k]|),  s[k] = float32(b sqrt(|ts[k+1] - ts[k]|))
 *   m_ref   = F_T mean + F_T cov inv(Kyy) (y - mean),  S_ref = F_T^2 cov + Q_T I - F_T cov inv(Kyy) F_T cov,
 *             Kyy = cov + obs_var I   (gp_csgm.py:69-76; the initial normal is multiplied by S_ref itself, as there)
 * built in float64 on the host and rounded once to float32 (fbs_amd/lg_csgm.py, lg_csgm_tables).
 *
 * Numeric specification (float32, no contraction beyond the chains named; tests/csgm_restate.py restates it in numpy):
 *   u0 == NULL (sample mode): key_init, key_sde = split(keys[b], 2); z = normal(key_init, (d,));
 *         u0[i]: acc = m_ref[i], then acc = fbsmi_fmaf(S_ref[i][c], z[c], acc) for c = 0..d-1
 *   u0 != NULL (integrate mode): keys[b] is key_sde, x = u0[b]
 *   step k: xi = normal(split(key_sde, T)[k], (1, d))[0]      (euler_maruyama's schedule with integration_nsteps = 1)
 *         f_i: acc = cvec[k][i], then acc = fbsmi_fmaf(A[k][i][c], x[c], acc) for c ascending
 *         x_i <- (x_i + f_i * ddt[k]) + s[k] * xi_i             (separate float32 operations)
 *   out[b] = x after step T-1;  path[0] = u0, path[k+1] = x after step k.
 * One kernel launch per fbsmi_csgm_run, on the caller's stream. */
typedef struct fbsmi_csgm_model {
    int32_t d, T;
    const float* A;     /* (T, d, d) */
    const float* cvec;  /* (T, d) */
    const float* ddt;   /* (T) */
    const float* s;     /* (T) */
    const float* m_ref; /* (d) */
    const float* S_ref; /* (d, d) */
} fbsmi_csgm_model;
typedef struct fbsmi_csgm fbsmi_csgm; /* opaque: the tables in the kernel's operand order, the u0 and path buffers */
/* B = nsamples trajectories per call.  The tables are read here, once (the handle keeps its own copy in the order the
 * kernel's matrix-core operands want).  d outside [1, 128] or nsamples outside [1, 131072]: FBSMI_ERR_UNSUPPORTED.
 * store_path: keep every step's state. */
int fbsmi_csgm_create(const fbsmi_csgm_model* model, int32_t nsamples, int store_path, fbsmi_csgm** out);
void fbsmi_csgm_destroy(fbsmi_csgm* h);
/* keys (B, 2); u0 (B, d) or NULL (see above); out (B, d). */
int fbsmi_csgm_run(fbsmi_csgm* h, const uint32_t* keys, const float* u0, float* out, void* stream);
/* State of the last run, copied to dst (nullable: only *count is set): which 0 the initial states u0 (B, d), 1 the
 * path (T+1, B, d) (store_path only). */
int fbsmi_csgm_view(fbsmi_csgm* h, int which, void* dst, int64_t* count, void* stream);

/* ---- batched, device-resident Kalman-filter conditional sampler for the analytic model ------------
 * The exact counterpart of fbsmi_lg_fsamp: the discretised model that bootstrap_filter targets is linear-Gaussian,
 *   u_0 | v_0 ~ N(m_0, Sigma_0)  (ref_sampler),   (u_{k+1}; v_{k+1}) | u_k, v_k ~ N(M_k (u_k; v_k) + dt g[k], sd[k]^2 I),
 * with the likelihood of v_{k+1} given the PREVIOUS state and the state then propagated, so its filtering law
 * p(u_T | v_0..v_T) = N(m_T, cov_T) and its marginal likelihood p(v_1..v_T | v_0) are closed-form: the N -> infinity limit
 * of fbsmi_lg_fsamp's sample and the exact value of the -nell it estimates.  (experiments/toy/gp_kf.py differentiates the
 * observation mean with respect to v_prev and passes sqrt(dt) b where a covariance is expected; this is the exact
 * filter, not that recursion.  Flags, key schedule and output of the driver are gp_kf.py's.)
 * Tables (fbs_amd/lg_kalman.py, lg_kalman_tables; float64 on the host, rounded once to float32).  Step k leaves
 * t_prev = ts[k]; M_k = I + dt G[k] = [[A, B], [C, D]] with the u rows first, (c; e) = dt g[k], q = sd[k]^2, Sigma_0 the
 * conditional covariance of ref_sampler; the covariance recursion does not depend on the data:
 *   S = C Sigma C^T + q I,  K = Sigma C^T inv(S),  Sigma+ = Sigma - K S K^T,  Sigma <- A Sigma+ A^T + q I (symmetrised)
 *   H[k] = [C D] (dv, D),  e[k] (dv),  Pm[k] = [A B] (du, D),  c[k] (du),  AK[k] = A K (du, dv),
 *   W[k] = inv(lower Cholesky factor of S) (dv, dv),  lconst[k] = -(log det S + dv log 2 pi) / 2,
 *   Lt = transposed lower Cholesky factor of cov_T = Sigma after step T-1.
 * Numeric specification (float32, no contraction beyond the chains named; tests/kf_restate.py restates it in numpy),
 * sample b with key = keys[b]:
 *   keys          key_fwd, key_bwd, key_kf = split(key, 3)            (gp_kf.py:151; key_bwd is unused, as there)
 *   forward path  exactly the "forward path" line of fbsmi_lg_fsamp: r[0] = y0, r[k+1] = F[k] * r[k] + sqQ[k] * xi[k],
 *                 xi = normal(key_fwd, (T, dv)); vs[k] = r[T - k]
 *   m_0           exactly the float64 conditional mean of the ref_sampler block of fbsmi_lg_pmcmc with yT = vs[0],
 *                 rounded to float32
 *   step k        z = (m, vs[k])  (D values)
 *                 pred_i: acc = e[k][i], then acc = fbsmi_fmaf(H[k][i][c], z[c], acc), c ascending;
 *                 r_i = vs[k+1][i] - pred_i
 *                 m'_j : acc = c[k][j], then acc = fbsmi_fmaf(Pm[k][j][c], z[c], acc), c ascending, then continued with
 *                        acc = fbsmi_fmaf(AK[k][j][c], r[c], acc), c ascending
 *                 qv_i : acc = 0, then acc = fbsmi_fmaf(W[k][i][c], r[c], acc), c ascending
 *                 ss   : acc = 0, then acc = fbsmi_fmaf(qv_i, qv_i, acc), i ascending
 *                 ll <- ll + ((-0.5f * ss) + lconst[k]),  ll = 0 before step 0
 *   sample        zz = normal(key_kf, (du,));  x_j: acc = m_T[j], then acc = fbsmi_fmaf(Lt[c][j], zz[c], acc), c ascending
 *                 (mean + zz @ chol)
 *   outputs       samples[b] = x, means[b] = m_T, loglik[b] = ll.
 * A call is two plain launches on the caller's stream (the front: keys, path, m_0; the recursion and the draw), nothing
 * on the host inside it. */
typedef struct fbsmi_kf_model {
    int32_t du, dv, T;
    const float* H;      /* (T, dv, du + dv) */
    const float* e;      /* (T, dv) */
    const float* Pm;     /* (T, du, du + dv) */
    const float* c;      /* (T, du) */
    const float* AK;     /* (T, du, dv) */
    const float* W;      /* (T, dv, dv) */
    const float* lconst; /* (T) */
    const float* Lt;     /* (du, du) */
    const float* F;      /* (T) the front: fbsmi_lg_model's F, sqQ and fbsmi_lg_pmcmc_tables' m_u, m_v, gain */
    const float* sqQ;    /* (T) */
    const double* m_u;   /* (du) */
    const double* m_v;   /* (dv) */
    const double* gain;  /* (du, dv) */
} fbsmi_kf_model;
typedef struct fbsmi_kf fbsmi_kf; /* opaque: the tables in the kernel's operand order, the vs and m_0 buffers */
/* B = nsamples samples per call.  The tables are device arrays, read here, once (the handle keeps its own copies).
 * FBSMI_ERR_ARG for a null model, T < 1 or a null table; FBSMI_ERR_UNSUPPORTED for du or dv outside [1, 128] or nsamples
 * outside [1, 65535]; all of this is answered before any device call. */
int fbsmi_kf_create(const fbsmi_kf_model* model, int32_t nsamples, fbsmi_kf** out);
void fbsmi_kf_destroy(fbsmi_kf* h);
/* keys (B, 2) and y0 (dv) are device inputs; samples (B, du), means (B, du) (nullable) and loglik (B) (nullable) device
 * outputs.  FBSMI_ERR_UNSUPPORTED for a model without an exact forward transition (F and sqQ all-zero placeholders), as
 * fbsmi_lg_fsamp_create answers. */
int fbsmi_kf_sample(fbsmi_kf* h, const uint32_t* keys, const float* y0, float* samples, float* means, float* loglik,
                    void* stream);
/* The filter alone on the caller's observation paths vs (B, T+1, dv), read in place: m_0 from vs[b][0], the T steps,
 * means (B, du) and loglik (B) (each nullable); nothing is drawn. */
int fbsmi_kf_filter(fbsmi_kf* h, const float* vs, float* means, float* loglik, void* stream);
/* State of the last call, copied to dst (nullable: only *count is set): which 0 vs (B, T+1, dv), the observation paths
 * of the last fbsmi_kf_sample; 1 m_ (B, du), the initial means m_0 of the last call of either kind. */
int fbsmi_kf_view(fbsmi_kf* h, int which, void* dst, int64_t* count, void* stream);
/* A model whose forward process is Euler-Maruyama (the Gaussian Schrodinger bridge, experiments/sb/filter.py:137-148): its
 * discretised reverse model is linear-Gaussian like the analytic one, so lg_kalman_tables applies to its G, g, sd, dt and
 * fbsmi_kf_create takes the all-zero F, sqQ placeholders; fbsmi_kf_filter serves such a handle as it is.  After this call
 * fbsmi_kf_sample serves it too: the front launch is the front of fbsmi_lg_fsamp_create_em, exactly its "keys" (key_fwd,
 * key_x0, key_em), "x0" and "forward path" lines -- the same keys give the same vs, bit for bit -- and m_0, the step, the
 * sample line (key_kf = split(key, 3)[2]) and the outputs are those of fbsmi_kf_sample above.  `fwd` covers the handle's T
 * and D = du + dv and must outlive it; x0_mean (du) and x0_chol (du, du), the LOWER factor, are device float32 arrays, both
 * null for x0 ~ N(0, I) ('heuristic') or both set ('proper'): the handle copies them, and for T > 1024 allocates the
 * (B, T, 2) interval keys.  FBSMI_ERR_ARG (before any device call) for a null handle or fwd, a null array in fwd,
 * fwd->nsub < 1, and exactly one of x0_mean / x0_chol null; FBSMI_ERR_UNSUPPORTED for a handle whose F, sqQ are not all
 * zero (it has an exact forward transition).  Without this call fbsmi_kf_sample answers such a handle as before. */
int fbsmi_kf_set_em_forward(fbsmi_kf* h, const fbsmi_em_forward* fwd, const float* x0_mean, const float* x0_chol);

/* ---- batched, device-resident Kalman smoother and path sampler for the analytic model ---------------
 * The exact counterpart of fbsmi_lg_backsim, as fbsmi_kf is of fbsmi_lg_fsamp: the smoothing law
 * p(u_0..u_T | v_0..v_T) of the model above is Gaussian, and a draw from it is the forward filter followed by a backward
 * sampler (Rauch-Tung-Striebel with noise).  Given u_{k+1} and v_0..v_T, u_k depends on (u_{k+1}, v_0..v_{k+1}) only
 * (u_{k+1} and v_{k+2} depend on (u_{k+1}, v_{k+1}) only and the u and v noises are independent), so with m_k, Sigma_k the
 * filtering moments before step k, r_k its innovation and Sigma_k+ = Sigma_k - K S K^T:
 *   u_T ~ N(m_T, cov_T),   u_k = m_k + K_k r_k + J_k (u_{k+1} - m_{k+1}) + Lb_k xi_k,   k = T-1 .. 0.
 * Tables (fbs_amd/lg_kalman.py, lg_smoother_tables; float64 on the host, rounded once to float32), per step k:
 *   K[k] = Sigma_k C^T inv(S) (du, dv),   J[k] = Sigma_k+ A^T inv(Sigma_{k+1}) (du, du),
 *   Lb[k] = lower Cholesky factor of Sigma_k+ - J Sigma_{k+1} J^T (symmetrised) (du, du), its upper triangle stored as zero.
 * Numeric specification (float32, no contraction beyond the chains named; tests/kfs_restate.py restates it in numpy),
 * sample b with key = keys[b]; the deviation delta_k = u_k - m_k is carried, not u_k:
 *   keys          key_fwd, key_bwd, key_kf = split(key, 3)
 *   front, m_0    exactly those of fbsmi_kf_sample (fbsmi_kf_filter when vs is the caller's)
 *   forward       exactly the step of fbsmi_kf, in the same chains; every m_k (k = 0..T) and r_k (k = 0..T-1) is kept;
 *                 loglik is fbsmi_kf's
 *   u_T           exactly the sample line of fbsmi_kf (zz = normal(key_kf, (du,)), the chain from m_T over Lt):
 *                 paths[b][T] = u_T;  delta_T = u_T - m_T
 *   noise         xi = normal(key_bwd, (T, du)); step k uses xi[k]
 *   step k        k = T-1 .. 0, every j: acc = 0;
 *                 acc = fbsmi_fmaf(K[k][j][c], r_k[c], acc), c ascending;
 *                 acc = fbsmi_fmaf(Lb[k][j][c], xi[k][c], acc), c ascending over all of [0, du);
 *                 acc = fbsmi_fmaf(J[k][j][c], delta_{k+1}[c], acc), c ascending;
 *                 delta_k[j] = acc;  paths[b][k][j] = m_k[j] + delta_k[j]
 *   smooth        delta_T = 0 (smeans[b][T][j] = m_T[j] + 0), the Lb line is left out, nothing is drawn.
 * A call is three plain launches on the caller's stream (the front; the forward recursion with stores; the backward
 * pass), nothing on the host inside it. */
typedef struct fbsmi_kfs_model {
    const fbsmi_kf_model* kf;
    const float* K;  /* (T, du, dv) */
    const float* J;  /* (T, du, du) */
    const float* Lb; /* (T, du, du) */
} fbsmi_kfs_model;
typedef struct fbsmi_kfs fbsmi_kfs; /* opaque: a filter handle of its own, the packed K, J, Lb, the m_k, r_k and u_T buffers */
/* Argument checks and limits are fbsmi_kf_create's, answered before any device call. */
int fbsmi_kfs_create(const fbsmi_kfs_model* model, int32_t nsamples, fbsmi_kfs** out);
void fbsmi_kfs_destroy(fbsmi_kfs* h);
/* keys (B, 2), y0 (dv): the observation paths are the handle's own front's, as in fbsmi_kf_sample (and refused alike for a
 * model without F, sqQ).  paths (B, T+1, du); loglik (B) nullable. */
int fbsmi_kfs_sample(fbsmi_kfs* h, const uint32_t* keys, const float* y0, float* paths, float* loglik, void* stream);
/* The same draw on the caller's observation paths vs (B, T+1, dv), read in place. */
int fbsmi_kfs_sample_on(fbsmi_kfs* h, const uint32_t* keys, const float* vs, float* paths, float* loglik, void* stream);
/* The smoothed means E[u_k | v_0..v_T] (B, T+1, du) on the caller's vs; nothing is drawn. */
int fbsmi_kfs_smooth(fbsmi_kfs* h, const float* vs, float* smeans, float* loglik, void* stream);
/* State of the last call, copied to dst (nullable: only *count is set): which 0 vs (B, T+1, dv), the observation paths of
 * the last fbsmi_kfs_sample; 1 the filter means m_k (B, T+1, du); 2 the innovations r_k (B, T, dv). */
int fbsmi_kfs_view(fbsmi_kfs* h, int which, void* dst, int64_t* count, void* stream);
/* fbsmi_kf_set_em_forward on the smoother's filter handle, with its checks and answers: afterwards fbsmi_kfs_sample draws
 * the observation paths by the Euler-Maruyama front (noise xi from key_bwd = split(key, 3)[1], as above). */
int fbsmi_kfs_set_em_forward(fbsmi_kfs* h, const fbsmi_em_forward* fwd, const float* x0_mean, const float* x0_chol);

/* ---- fused SMC step for score-network models (image experiments) --------------------------------
 * The three closures of experiments/imgs/inpainting.py:102-147 (and supr.py; sb_imgs/supr.py:80-127)
 * wrap ONE network evaluation on the joint image concat(u, v) per SMC step (csmc.py:142,145 evaluate it
 * twice on the same input).  Around that evaluation (PyTorch-ROCm, not part of this library) the step is
 * two kernels:
 *   fbsmi_em_concat : ancestor gather (csmc.py:140) + ImageRestore.concat (fbs/data/images.py:355-363)
 *                     -> the network's input, written once in the network's dtype;
 *   fbsmi_em_finish : ImageRestore.unpack of the network output (images.py:333-353), reverse drift
 *                     (inpainting.py:102-103), Euler-Maruyama proposal with in-kernel
 *                     jax.random.normal (inpainting.py:122-128), reference pin (csmc.py:143) and the
 *                     row-summed Gaussian log-density of the observed increment (inpainting.py:141-147).
 * A particle row holds du unobserved floats (p, c) -> p*c + channel; an image holds D = du + dv floats
 * (w, h, c) row-major.  The mask is three int32 device tables:
 *   u_off (du): image offset of unobserved element j;  v_off (dv): image offset of observed element j;
 *   role (D): inverse map, role[e] = j >= 0 if image element e is unobserved element j, ~j < 0 if it is
 *   observed element j.                                                                              */
typedef struct fbsmi_em_mask {
    int32_t du, dv;
    const int32_t* u_off;
    const int32_t* v_off;
    const int32_t* role;
} fbsmi_em_mask;

/* img[r] = concat(us[A[r]], v_prev) for n rows; A nullable (identity).  out_dtype 0 float32, 1 bfloat16
 * (round to nearest even).  us (rows, du), v_prev (dv), img (n, D). */
int fbsmi_em_concat(const fbsmi_em_mask* mask, const float* us, const int32_t* A, const float* v_prev, int64_t n,
                    int out_dtype, void* img, void* stream);

/* net: the network evaluated on fbsmi_em_concat's output, (rows, D); net_dtype 0 float32, 1 bfloat16.  Row r of
 * this call uses net[net_A[r]] (net_A nullable: net[r]) -- pmcmc_filter_step (fbs/samplers/smc.py:144-150)
 * weights the particles, resamples, and proposes from the SAME network input rows, gathered.
 * mode 0: reverse drift = cx * x + cs * net (score model: cx = -a(T - t), cs = b(T - t)^2, inpainting.py:102-103);
 * mode 1: reverse drift = net (Schrodinger-bridge backward drift, sb_imgs/supr.py:84-85).
 * With x = us[A[r]] (A nullable), z = rows [row0, row0 + n) of jax.random.normal(key, (n_total, du)):
 *   us_new[r] = (x + drift_u * dt) + sd * z;   us_new[pin_row] = pin_value (pin_row < 0: no pin);
 *   lw[r] = tree-sum_j ( log(2 pi sd^2) + (v[j] - (v_prev[j] + drift_v[j] * dt))^2 / sd^2 ) / -2
 * (jax.scipy.stats.norm.logpdf summed in the canonical pairwise order of include/fbsmi_math.h).
 * us_new (n, du) nullable (no proposal), lw (n) nullable (no weights); us_new must not alias us.
 * n_total * du <= 2^32 - 4 (FBSMI_ERR_ARG beyond: the flat index of the draw is 32 bits wide). */
int fbsmi_em_finish(const fbsmi_em_mask* mask, const float* us, const int32_t* A, const void* net,
                    const int32_t* net_A, int net_dtype, int mode, float cx, float cs, float dt, float sd, const float* v, const float* v_prev, uint32_t k0,
                    uint32_t k1, int64_t n_total, int64_t row0, int64_t n, int64_t pin_row, const float* pin_value,
                    float* us_new, float* lw, void* stream);

/* transition_logpdf (inpainting.py:131-138): lw[r] = sum_j norm.logpdf(u[j]; us[r][j] + drift_u[r][j] * dt, sd)
 * for the n rows of us (n, du) and the network output net (n, D) on concat(us, v_prev); u (du). */
int fbsmi_em_transition_logpdf(const fbsmi_em_mask* mask, const float* us, const void* net, int net_dtype, int mode,
                               float cx, float cs, float dt, float sd, const float* u, int64_t n, float* lw,
                               void* stream);

/* What a call of the three entry points above would launch, decided on the host from the mask's sizes and the VALUES of
 * the pointers (nothing is dereferenced, no HIP call is made: these run without a GPU).  Each *_plan function takes the
 * arguments of its entry point that the decision or an argument check reads, returns what the entry point would return
 * for them (FBSMI_ERR_ARG with the same message for a refused call), and fills *plan; the entry points themselves launch
 * from the same plan.  kernel NONE: the call returns FBSMI_OK without a launch (n == 0, or nothing asked for). */
#define FBSMI_EM_KERNEL_NONE 0
#define FBSMI_EM_KERNEL_FINISH 1   /* k_em_finish: proposal and log-density workgroups in one grid */
#define FBSMI_EM_KERNEL_ROWS 2     /* k_em_rows: one workgroup per row, the network row staged in LDS */
#define FBSMI_EM_KERNEL_TRANSLP 3  /* k_em_translp */
#define FBSMI_EM_KERNEL_CONCAT 4   /* k_em_concat */
typedef struct fbsmi_em_plan {
    int32_t kernel;      /* FBSMI_EM_KERNEL_* */
    int32_t pair;        /* finish: the call covers the whole draw, a thread takes both words of a Threefry call */
    int32_t vec;         /* finish, concat: the 16-byte variant (0: element by element) */
    int32_t ku;          /* rows: proposal groups per thread, 1..4; concat: chunks of 4096 elements per row */
    int32_t nU, nV;      /* finish: proposal / log-density workgroups; transition_logpdf: nV rows */
    int32_t vfirst;      /* finish: 1 log-density workgroups first, 0 the two roles interleaved over the grid */
    int32_t nseg;        /* 256-element segments of the summed part; above 64 the segment sums meet in an LDS tree */
    int32_t lnet_bytes;  /* rows: LDS bytes of the staged network row */
    int32_t lds_bytes;   /* dynamic LDS of the launch */
    int32_t grid;        /* workgroups of the launch */
} fbsmi_em_plan;
int fbsmi_em_concat_plan(const fbsmi_em_mask* mask, const void* us, const void* v_prev, int64_t n, int out_dtype,
                         const void* img, fbsmi_em_plan* plan);
int fbsmi_em_finish_plan(const fbsmi_em_mask* mask, const void* us, const void* net, int net_dtype, int mode, const void* v,
                         const void* v_prev, int64_t n_total, int64_t row0, int64_t n, int64_t pin_row,
                         const void* pin_value, const void* us_new, const void* lw, fbsmi_em_plan* plan);
int fbsmi_em_transition_logpdf_plan(const fbsmi_em_mask* mask, const void* us, const void* net, int net_dtype, int mode,
                                    const void* u, int64_t n, const void* lw, fbsmi_em_plan* plan);

/* ---- the closure tier for B ensembles in lockstep (fbs_amd/csrc/fbsmi_batch.hip) -----------------
 * B independent ensembles of n rows each (the test images of one run, the chains of one image) share the time grid, the
 * SDE and the network, so a step is ONE launch per sampler operation for all of them and one network call on B * n rows.
 * One workgroup per ensemble, everything of an ensemble in its LDS: no workspace.  1 <= n <= 1024; B is bounded by the
 * grid only.  Decided on the host before any HIP call: FBSMI_ERR_ARG for a null pointer, B < 1 or n < 1, nmasks outside
 * {1, B} and n * du > 2^32 - 4; FBSMI_ERR_UNSUPPORTED for n > 1024.
 *
 * Row b of out (B, n) = fbsmi_normalise on lw[b], bit for bit (the two-level logsumexp of include/fbsmi_math.h, sums in
 * the canonical tree over the element index); out_lse (B), nullable, receives the logsumexp of every row. */
int fbsmi_normalise_batched(const float* lw, int64_t B, int64_t n, int log_space, float* out, float* out_lse,
                            void* stream);
/* Row b of idx (B, n) = fbsmi_cond_resample(kind 1, keys[b], w[b], i[b], j[b], conditional = 1), bit for bit; the indices
 * are local to the ensemble.  keys (B, 2), w (B, n), i (B), j (B): device arrays. */
int fbsmi_cond_killing_batched(const uint32_t* keys, const float* w, const int32_t* i, const int32_t* j, int64_t B,
                               int64_t n, int32_t* idx, void* stream);

/* The masks of the B ensembles: nmasks == 1 (one mask for all) or nmasks == B; every mask has the same du and dv (the
 * inpainting rectangles of one size, the super-resolution masks of one rate).  Tables as in fbsmi_em_mask, stacked:
 * u_off (nmasks, du), v_off (nmasks, dv), role (nmasks, du + dv). */
typedef struct fbsmi_em_mask_batch {
    int32_t du, dv, nmasks;
    const int32_t* u_off;
    const int32_t* v_off;
    const int32_t* role;
} fbsmi_em_mask_batch;

/* Ensemble b = fbsmi_em_concat: img[b * n + r] = concat(us[b][A[b][r]], v_prev[b]).  us (B, n, du), A (B, n) nullable
 * (identity; ancestors local to the ensemble), v_prev (B, dv), img (B * n, D) float32 or bfloat16 (out_dtype 0 / 1). */
int fbsmi_em_concat_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const float* v_prev,
                            int64_t B, int64_t n, int out_dtype, void* img, void* stream);
/* Ensemble b = fbsmi_em_finish with n_total = n, row0 = 0, net_A = NULL, bit for bit: it draws normal(keys[b], (n, du))
 * exactly as a call of its own would.  net (B * n, D); v, v_prev (B, dv); keys (B, 2); pin_row (B) nullable, -1 = no pin
 * in that ensemble; pin_value (B, du); us_new (B, n, du) nullable (weights only), lw (B, n) nullable.  mode, cx, cs, dt,
 * sd are shared: the ensembles are at the same time step. */
int fbsmi_em_finish_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const void* net,
                            int net_dtype, int mode, float cx, float cs, float dt, float sd, const float* v,
                            const float* v_prev, const uint32_t* keys, int64_t B, int64_t n, const int32_t* pin_row,
                            const float* pin_value, float* us_new, float* lw, void* stream);

/* Row b of idx (B, n) = fbsmi_resample(kind, w[b], keys[b], n), bit for bit, for kind 0 (stratified) and 1 (systematic);
 * the indices are local to the ensemble.  keys (B, 2), w (B, n): device arrays.  One workgroup per ensemble, no
 * workspace.  kind 2 (multinomial) and 3 (killing) are FBSMI_ERR_UNSUPPORTED, any other kind FBSMI_ERR_ARG; otherwise the
 * refusals of fbsmi_normalise_batched. */
int fbsmi_resample_batched(int kind, const uint32_t* keys, const float* w, int64_t B, int64_t n, int32_t* idx,
                           void* stream);
/* The proposal half of a weight -> resample -> propose step (fbs/samplers/smc.py:144-150) on the network output the
 * weights were computed from: ensemble b = fbsmi_em_finish with A = net_A = A[b], n_total = n, row0 = 0, no pin, lw = NULL,
 * bit for bit.  Row r proposes from us[b][A[b][r]] with the network's output row b * n + A[b][r]; its noise is row r of
 * normal(keys[b], (n, du)).  A (B, n) is required and its entries are clamped into [0, n - 1]; us_new (B, n, du) must
 * not alias us.  Refusals as fbsmi_em_finish_batched. */
int fbsmi_em_propose_batched(const fbsmi_em_mask_batch* mask, const float* us, const int32_t* A, const void* net,
                             int net_dtype, int mode, float cx, float cs, float dt, float sd, const uint32_t* keys,
                             int64_t B, int64_t n, float* us_new, void* stream);

/* One step of the image CSGM sampler (fbs_amd/csgm.py; experiments/imgs/inpainting_csgm.py:88-113) for B independent
 * trajectories in ONE launch: a workgroup per trajectory, a thread per image position, no LDS and no workspace.  With
 * o = role[e] the (u, v) element of image position e < D = du + dv:
 *   o >= 0 (unobserved), net given:  x = u[b][o], s = net[b * D + e] (float32, or bfloat16 widened; net_dtype 0 / 1),
 *       t1 = cx * x, t2 = cs * s, d = t1 + t2, m = x + d * dt, nz = c * z, out = m + nz   -- every operation rounded
 *       separately -- with z = element noise_offset + o of normal(scan_keys[b], (noise_total,)): fbsmi_em_update on the
 *       drift -(a u) + b^2 s, bit for bit.  u_new[b][o] = out, and img[b][e] = out when img is given.
 *   o >= 0, net == NULL:  img[b][e] = u[b][o].
 *   o < 0 (observed, j = ~o), img given:  img[b][e] = (F * y0[b][j]) + (sq * zj), zj = element j of
 *       normal(est_keys[b], (dv,)).
 * img (B, D) is float32 or bfloat16 rounded to nearest even (out_dtype 0 / 1) and may be NULL (the last step: update
 * only); net (B, D) may be NULL (the first launch: network input only).  u, u_new (B, du) may be the same array; y0
 * (B, dv); scan_keys, est_keys (B, 2) device arrays, both required.  Table entries are clamped into their part before
 * they address memory.  Decided on the host before any HIP call, FBSMI_ERR_ARG: a null mask, table, u, y0 (dv > 0) or
 * key array; neither net nor img; net without u_new; B outside [1, 2^31 - 1] (no cap on rows otherwise); nmasks outside
 * {1, B}; a dtype flag outside {0, 1}; noise_offset < 0 or noise_offset + du > noise_total; noise_total > 2^32 - 4 (the
 * draw primitive's counters are 32 bits wide, as in fbsmi_em_finish). */
int fbsmi_em_csgm_step_batched(const fbsmi_em_mask_batch* mask, const float* u, const void* net, int net_dtype, float cx,
                               float cs, float dt, float c, const uint32_t* scan_keys, int64_t noise_total,
                               int64_t noise_offset, const float* y0, float F, float sq, const uint32_t* est_keys,
                               int out_dtype, void* img, int64_t B, float* u_new, void* stream);
/* Row b of out (B, n) = fbsmi_normal(keys[b], n), bit for bit, in one launch.  keys (B, 2): device array.  FBSMI_ERR_ARG
 * for a null pointer, B < 1, n < 0, n > 2^32 - 4 or more workgroups than one grid holds; n == 0 launches nothing. */
int fbsmi_normal_batched(const uint32_t* keys, int64_t B, int64_t n, float* out, void* stream);
/* Row b of out (B) = fbsmi_categorical(keys[b], w[b], n), bit for bit, in one launch: one workgroup per ensemble, the CDF
 * tree in LDS, no workspace.  keys (B, 2), w (B, n): device arrays.  Refusals as fbsmi_normalise_batched. */
int fbsmi_categorical_batched(const uint32_t* keys, const float* w, int64_t B, int64_t n, int32_t* out, void* stream);

/* ---- the forward noising paths of B ensembles in lockstep (ScoreBridge.fwd_sampler_batched / fwd_ys_sampler_batched) ----
 * The state of ensemble b is an image of D = du + dv floats in image order; its path is written ALREADY UNPACKED.  With
 * o = role[e] of image position e:  o >= 0 is element o of the u output, o < 0 element ~o of the v output, each addressed
 * as base + slot * slot_stride + b * b_stride + element (strides in floats, chosen by the caller: (T + 1, B, du) and
 * (B, T + 1, du) are both one launch, and no concat, unpack, flip or stack follows).  out_v may be NULL: the observed
 * half is then not written.  mask may be NULL: the identity layout, every position goes to the u output, du = D, y0s is
 * not read.  With a mask, D must equal du + dv; only its role table is read, and its entries are clamped into their part
 * before they address memory.  x0s (B, du), y0s (B, dv), keys (B, 2): device arrays.
 *
 * Decided on the host before any HIP call, FBSMI_ERR_ARG: a mask without its role table, with du < 1 or dv < 0; D outside
 * [1, 2^31 - 1] or not du + dv; B outside [1, 2^31 - 1]; nmasks outside {1, B}; a null array the call reads or writes; a
 * dtype flag outside {0, 1}; a draw longer than 2^32 - 4; more workgroups (min(ceil(D / block), 64) per ensemble) than one
 * grid holds.
 *
 * linear_path: B whole paths in one launch.  Point 0 of ensemble b is the image assembled from x0s[b] and y0s[b] through
 * role; then x <- F[k] * x + S[k] * xi for k < T (the product F[k] * x, the product S[k] * xi and their sum each rounded
 * separately), xi = element k * D + e of normal(keys[b], (T * D,)) drawn in the kernel: fbsmi_linear_path on
 * normal(keys[b], (T, D)) bit for bit.  Point k lands in slot T - k when `reverse` is set, else in slot k.  F, S (T):
 * float32 device tables shared by the ensembles.  64-thread workgroups; a thread owns one (b, e) and walks the T steps.
 * Also refused: T < 0, null F or S with T > 0, T * D > 2^32 - 4. */
int fbsmi_linear_path_batched(const fbsmi_em_mask_batch* mask, int64_t D, const float* F, const float* S, const float* x0s,
                              const float* y0s, const uint32_t* keys, int64_t B, int32_t T, int reverse, float* out_u,
                              int64_t u_slot_stride, int64_t u_b_stride, float* out_v, int64_t v_slot_stride,
                              int64_t v_b_stride, void* stream);
/* em_fwd_step: one Euler-Maruyama sub-step of B image-shaped paths in one launch; x, x_out (B, D) float32 in image order
 * (x_out may be x; as (B, w, h, c) it is itself the next network input).
 *   net == NULL (the first launch): x_out[b] = the image assembled from x0s[b] and y0s[b] through role; x and keys are not
 *       read.
 *   otherwise:  m = x + f * ddt,  nz = c * xi,  out = m + nz  -- every operation rounded separately -- with f = net[b][e]
 *       (float32, or bfloat16 widened; net_dtype 0 / 1) and xi = element noise_offset + e of
 *       normal(keys[b], (noise_total,)): fbsmi_em_update bit for bit, per ensemble.  x0s, y0s are not read.
 * When store_slot >= 0 the result also goes to slot store_slot of the path outputs (out_u is then required).
 * Also refused: null x_out; net without x or keys; net == NULL without x0s (y0s when dv > 0); noise_offset < 0 or
 * noise_offset + D > noise_total; noise_total > 2^32 - 4. */
int fbsmi_em_fwd_step_batched(const fbsmi_em_mask_batch* mask, int64_t D, const float* x0s, const float* y0s, const float* x,
                              const void* net, int net_dtype, float ddt, float c, const uint32_t* keys, int64_t noise_total,
                              int64_t noise_offset, int64_t B, float* x_out, int64_t store_slot, float* out_u,
                              int64_t u_slot_stride, int64_t u_b_stride, float* out_v, int64_t v_slot_stride,
                              int64_t v_b_stride, void* stream);

/* ---- the rest of a Gibbs sweep for B ensembles in lockstep (fbs_amd/samplers/gibbs_batched.py): the forced move, the
 * fresh reference indices, the backward scanning pass and the Doob bridge of marg_y.  Each is its single-ensemble entry
 * point per ensemble, bit for bit, in one launch.  keys, w, k, log_w_T, As, uss, target, x0: device arrays. ----
 *
 * force_move: out_i[b] = fbsmi_force_move(keys[b], w[b], k[b], n)'s index (gibbs.py:171-214).  With w_k = w[b][k],
 * temp = 1 - w_k:  rest_e = (e == k ? 0 : w_e) / temp when w_k < 1, else float32(1.0 / n);  cdf = the canonical-tree scan
 * of rest (fbsmi_cumsum's);  (ka, kb) = split(keys[b], 2);  i = searchsorted_left(cdf, cdf[n - 1] * (1 - uniform(ka, ())));
 * u = uniform(kb, ());  out_i = u * (1 - w_i) < temp ? i : k.  out_alpha, nullable, receives
 * clip(tree-sum_e nan_to_zero(temp * rest_e / (1 - w_e)), 0, 1) and costs nothing when NULL.  One workgroup per ensemble,
 * 1 <= n <= 1024.  k[b] outside [0, n) is clamped before it addresses memory, and so is i.  Refusals as
 * fbsmi_normalise_batched. */
int fbsmi_force_move_batched(const uint32_t* keys, const float* w, const int32_t* k, int64_t B, int64_t n, int32_t* out_i,
                             float* out_alpha, void* stream);
/* Row b of out (B, n) = fbsmi_randint(keys[b], n, lo, hi), bit for bit, in one launch; any n (min(ceil(n / 256), 64)
 * workgroups per row).  FBSMI_ERR_ARG for a null pointer, B < 1, n < 0, n > 2^32 - 4 or more workgroups than one grid
 * holds; n == 0 launches nothing. */
int fbsmi_randint_batched(const uint32_t* keys, int64_t B, int64_t n, int32_t lo, int32_t hi, int32_t* out, void* stream);
/* backscan: ensemble b = backward_scanning_pass(keys[b], As[:, b], uss[:, b], log_w_T[b]) (csmc.py:230-270):
 *   w = fbsmi_normalise(log_w_T[b], log_space = 0) with the arithmetic of fbsmi_normalise_batched;
 *   Bs[b][T] = fbsmi_categorical(keys[b], w);  Bs[b][k - 1] = As[k - 1][b][Bs[b][k]] for k = T .. 1 (fbsmi_backtrace);
 *   path[b][k] = uss[k][b][Bs[b][k]] for k = 0 .. T.
 * As (T, B, n) int32 and uss (T + 1, B, n, du) are TIME-major, the way the forward pass produces them; Bs (B, T + 1) int32
 * and path (B, T + 1, du) are batch-major.  One workgroup per ensemble: one thread walks the trace and parks it in Bs,
 * after a barrier all threads copy the rows.  Every index is clamped into [0, n) before it addresses memory.  T = 0 is
 * allowed (As is then not read).  FBSMI_ERR_ARG for a null pointer, T < 0, B, n or du < 1; FBSMI_ERR_UNSUPPORTED for
 * n > 1024. */
int fbsmi_backscan_batched(const uint32_t* keys, const float* log_w_T, const int32_t* As, const float* uss, int64_t B,
                           int64_t n, int32_t T, int64_t du, int32_t* Bs, float* path, void* stream);
/* affine_em_path: ensemble b = fbsmi_affine_em_path(keys[b], A, Bt, S, ddt, target[b], x0[b], T, nsub, D, replace_last),
 * the same expression under the same contraction setting (the numeric specification restated at
 * fbsmi_lg_sweep_set_bridge); the tables A, Bt, S (T * nsub) and ddt (T) are shared by the ensembles.  keys (B, T, 2),
 * target, x0 (B, D).  Point k of ensemble b is written at out + (reverse ? T - k : k) * slot_stride + b * ens_stride
 * (strides in floats): the reversed, time-major observation path of a sweep needs no flip and no stack.  64-thread
 * workgroups, min(ceil(D / 64), 64) per ensemble, any D >= 1.  FBSMI_ERR_ARG for a null pointer the call reads, T < 0,
 * nsub < 1, D < 1, B outside [1, 2^31 - 1], nsub * D > 2^32 - 4, a negative stride or more workgroups than one grid holds. */
int fbsmi_affine_em_path_batched(const uint32_t* keys, const float* A, const float* Bt, const float* S, const float* ddt,
                                 const float* target, const float* x0, int32_t T, int32_t nsub, int64_t D, int replace_last,
                                 int64_t B, float* out, int64_t slot_stride, int64_t ens_stride, int reverse, void* stream);

/* ---- backward simulation for B ensembles in lockstep (bootstrap_backward_smoother_batched, smc.py:91-112;
 * backward_sampling_pass_batched, csmc.py:167-227): a step is one em_translp launch and one backsim_pick launch for all
 * ensembles, and nothing is read back between them. ----
 *
 * em_translp: lw[b][r] = fbsmi_em_transition_logpdf of ensemble b alone, bit for bit:
 *   tree-sum over the unobserved index j in [0, du) of nlp(u[b][j], x + drift * dt, sd * sd),  x = us[b][r][j],
 *   drift = (cx * x) + (cs * s) (mode 0) or s (mode 1),  s = net[(b * n + r) * D + u_off[j]] (float32, or bfloat16 widened;
 *   net_dtype 0 / 1), with nlp and the tree-sum as defined for the image twisted SMC below (the summation of
 *   fbsmi_em_finish_batched's log-weights).  Row (b, r) of the particles is at us + b * us_ens_stride + r * du and the
 *   target of ensemble b at u + b * u_ens_stride (strides in floats): a time slice of a batch-major (B, T + 1, n, du) or a
 *   time-major (T + 1, B, n, du) particle array, and a slot of a (B, T + 1, du) trajectory, are read in place.  net
 *   (B * n, D), lw (B, n).  One workgroup of 256 threads per row; table entries are clamped into [0, D) before they
 *   address memory.  FBSMI_ERR_ARG for a null pointer, B < 1, n < 1, du < 1, nmasks outside {1, B}, a flag outside {0, 1},
 *   a negative stride and B * n > 2^31 - 1; FBSMI_ERR_UNSUPPORTED for n > 1024 and du > 2^20.  Nothing is launched then. */
int fbsmi_em_translp_batched(const fbsmi_em_mask_batch* mask, const float* us, int64_t us_ens_stride, const void* net,
                             int net_dtype, int mode, float cx, float cs, float dt, float sd, const float* u,
                             int64_t u_ens_stride, int64_t B, int64_t n, float* lw, void* stream);
/* backsim_pick: for ensemble b,
 *   g = lw[b];  with log_w given:  m = max_r g[r],  g[r] = (g[r] - m) + log_w[b][r]  (two roundings, in this order);
 *   w = fbsmi_normalise(g, log_space = 0) with the arithmetic of fbsmi_normalise_batched;
 *   i = fbsmi_categorical(keys[b], w), clamped into [0, n);  idx[b * idx_stride] = i;
 *   out[b * out_ens_stride + c] = us[b * us_ens_stride + i * du + c] for c in [0, du).
 * keys (B, 2), lw and log_w (B, n) contiguous, log_w nullable; strides in floats / ints: idx may be a column of a
 * (B, T + 1) array and out a slot of a (B, T + 1, du) trajectory.  One workgroup of next_pow2(n) (at least 64) threads
 * per ensemble, everything in LDS; every thread reaches every barrier.  FBSMI_ERR_ARG for a null pointer (but log_w),
 * B, n or du < 1, or a negative stride; FBSMI_ERR_UNSUPPORTED for n > 1024. */
int fbsmi_backsim_pick_batched(const uint32_t* keys, const float* lw, const float* log_w, const float* us,
                               int64_t us_ens_stride, int64_t B, int64_t n, int64_t du, int32_t* idx, int64_t idx_stride,
                               float* out, int64_t out_ens_stride, void* stream);

/* ---- the step of the image twisted SMC for B ensembles in lockstep (fbs_amd/twisted.py make_image_twisted_batched;
 * experiments/imgs/inpainting_twisted.py:97-154; score mode only) ----
 * Particles are whole images: X (B * n, D) float32 in image order, D = du + dv = w * h * c, row b * n + r = particle r of
 * ensemble b.  role[e] < 0: image element e is observed element ~role[e] of y (B, dv); v_off[j] is the image element of
 * observed element j.  net (B * n, D) is the score at the rows of the X it comes with, float32 or bfloat16 widened
 * (net_dtype 0 / 1).  cx = -a(s), cs = b(s)^2, dt, sd = sqrt(dt) b(s), var_y = F(s)^2 data_variance + Q(s) at the forward
 * time s = T - t of the step: float64 on the host, rounded to float32.  One workgroup of 256 threads per row.
 *
 * Every operation below is one float32 operation, rounded to nearest, in the order written (no fused multiply-add):
 *   t1 = cx * x,  t2 = cs * s,  rd = t1 + t2,  p = rd * dt,  den = x + p                 (the one-step denoising estimate)
 *   nlp(a, m, v):  df = a - m,  sq = df * df,  q = sq / v,  (fbsmi_logf(6.2831855f * v) + q) * -0.5f
 *   g = (y[b][~role[e]] - den_e) / var_y on an observed element e, 0 elsewhere
 * A row sum ("tree-sum") over an index i in [0, d) is the canonical pairwise tree of include/fbsmi_math.h over i, zero
 * padded: four consecutive elements in a thread ((t0 + t1) + (t2 + t3)), six levels in the wave, the 256-element segment
 * sums in LDS and the same tree over the segments.  Table entries are clamped into their range before they address
 * memory, ancestors into [0, n - 1].
 *
 * Decided on the host before any HIP call: FBSMI_ERR_ARG for a null pointer (mask, tables, or any array the call needs),
 * B < 1, n < 1, nmasks outside {1, B}, a dtype flag outside {0, 1}, n * D > 2^32 - 4 and B * n > 2^31 - 1;
 * FBSMI_ERR_UNSUPPORTED for n > 1024 and D > 2^20.
 *
 * gather: Xp[b][r] = X[b][A[b][r]] and, when lp_prev_g is given, lp_prev_g[b][r] = lp[b][A[b][r]].  Xp (float32: the
 * autograd leaf) must not alias X.  D is passed as a number: no mask is read. */
int fbsmi_tw_img_gather_batched(const float* X, const float* lp, const int32_t* A, int64_t B, int64_t n, int64_t D,
                                float* Xp, float* lp_prev_g, void* stream);
/* twist: lp[row] = tree-sum over the observed index j in [0, dv) of nlp(y[b][j], den_{v_off[j]}, var_y) (0 for dv == 0).
 * With lw given (tl, pl, lp_prev_g (B * n) are then required):  s1 = tl + lp,  s2 = s1 - pl,  lw = s2 - lp_prev_g  -- the
 * unnormalised log-weights of a step; without it, the initial ones. */
int fbsmi_tw_img_twist_batched(const fbsmi_em_mask_batch* mask, const float* X, const void* net, int net_dtype, float cx,
                               float cs, float dt, float var_y, const float* y, const float* tl, const float* pl,
                               const float* lp_prev_g, int64_t B, int64_t n, float* lp, float* lw, void* stream);
/* cotangent: ct[row][e] = (cs * dt) * g_e, float32 (B * n, D): d lp / d net, the output cotangent of the network's
 * vector-Jacobian product. */
int fbsmi_tw_img_cotangent_batched(const fbsmi_em_mask_batch* mask, const float* X, const void* net, int net_dtype,
                                   float cx, float cs, float dt, float var_y, const float* y, int64_t B, int64_t n,
                                   float* ct, void* stream);
/* propose: with vjp (B * n, D) float32 = the vector-Jacobian product of the network at Xp with cotangent ct,
 *   c1 = cx * dt,  kap = 1 + c1,  hg = kap * g,  grad = hg + vjp       (d lp / d x: the head in closed form + the network)
 *   cg = cs * grad,  cd = rd + cg,  pm = cd * dt,  m = x + pm          (the twisted proposal's mean)
 *   nz = sd * z,  x_new = m + nz,  z = element r * D + e of normal(keys[b], (n * D,)) = of normal(keys[b], (n, w, h, c))
 *   var = sd * sd;  tl[row] = tree-sum over e in [0, D) of nlp(x_new, den, var)     (the transition density)
 *                   pl[row] = tree-sum over e in [0, D) of nlp(x_new, m, var)       (the proposal density)
 * X_new (B * n, D) float32 must not alias Xp; X_new_net, nullable, receives a copy of X_new in float32 or bfloat16 rounded
 * to nearest even (out_dtype 0 / 1): the input of the next network call.  keys (B, 2): device array. */
int fbsmi_tw_img_propose_batched(const fbsmi_em_mask_batch* mask, const float* Xp, const void* net, int net_dtype,
                                 const float* vjp, float cx, float cs, float dt, float sd, float var_y, const float* y,
                                 const uint32_t* keys, int64_t B, int64_t n, float* X_new, float* tl, float* pl,
                                 int out_dtype, void* X_new_net, void* stream);

/* ---- image metrics (fbs_amd/image_metrics.py; the paper's Tables 2 and 3 and Figure 8) ----
 * All statistics are float64; the inputs are float32, so their products are exact in float64.  No operation is fused.
 *
 * psnr_ssim: true_imgs (G, H, W, C), restored (G, S, H, W, C), psnr and ssim (G, S) float64; image (g, s) is scored
 * against true image g.  clip = 1 first maps every value v of both images to 0 for v < 0 and 1 for v > 1; data_range is 1.
 *   PSNR = 10 log10(1 / mse),  mse = (sum of (x - y)^2 over the H W C elements) / (H W C);  mse == 0 gives +inf.
 *   SSIM, per channel, over the (H - 6)(W - 6) 7x7 windows that lie inside the image, n = 49:
 *     ux = sum x / n, uy = sum y / n,  vx = n/(n-1) (sum xx / n - ux ux), vy and vxy likewise (sample covariances),
 *     C1 = 0.01^2, C2 = 0.03^2,  S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux ux + uy uy + C1)(vx + vy + C2)),
 *   the mean of S over the windows, then the mean over the channels.  Equal images give exactly 1.
 * Every sum has a fixed order that depends on (H, W, C) alone: the result for image (g, s) has the same bits in any call.
 * ws: fbsmi_img_psnr_ssim_workspace_bytes(G * S, H, W, C) bytes of device scratch (0 for an unsupported shape).
 * FBSMI_ERR_ARG for a null pointer, G or S < 1, clip outside {0, 1} or more than 2^31 - 1 workgroups;
 * FBSMI_ERR_UNSUPPORTED outside 7 <= H, W <= 256 and 1 <= C <= 4.  Nothing is launched then. */
size_t fbsmi_img_psnr_ssim_workspace_bytes(int64_t GS, int32_t H, int32_t W, int32_t C);
int fbsmi_img_psnr_ssim_batched(const float* true_imgs, const float* restored, int64_t G, int64_t S, int32_t H, int32_t W,
                                int32_t C, int clip, double* psnr, double* ssim, void* ws, void* stream);
/* chain autocorrelation: chains (M, S, D) float32, ac (M, L, D) and best (M, L) float64, 1 <= L <= S.  For variable d of
 * chain m, with c_t = x_t - (sum_t x_t) / S and sums over t ascending:
 *   ac[k] = ((sum over t < S - k of c_t c_{t+k}) / (S - k)) / ((sum_t c_t c_t) / S)
 * (the unbiased estimator, as a direct sum).  A variable whose S samples all have the same bits is constant: its ac is NaN
 * at every lag.  best[m][k] = the minimum over the non-NaN variables of max(ac[m][k][d], 0), NaN when there is none.
 * FBSMI_ERR_ARG for a null pointer, M, S or D < 1 or L outside [1, S]; FBSMI_ERR_UNSUPPORTED for M > 65535, S > 2^20 or
 * D > 2^24. */
int fbsmi_chain_autocorr_batched(const float* chains, int64_t M, int64_t S, int64_t D, int64_t L, double* ac, double* best,
                                 void* stream);

/* ---- the denoising score-matching trainer (fbs_amd/sdes/losses.py make_linear_sde_law_loss, fbs_amd/train.py) ----
 * fbs/sdes/linear.py:230-360 and fbs/nn/utils.py:60-83 round the network.  Every product, sum and quotient below is one
 * float32 operation rounded on its own (-ffp-contract=off); tree_sum is the root of the pairwise tree over the zero-padded
 * element index, the tree of fbsmi_sum, whatever the tiling.  bfloat16 values are widened exactly on load and rounded to
 * nearest even on store.  Everything is refused on the host before any HIP call, and nothing is launched then. */

/* fbsmi_uniform(key, n) on the HOST, bit for bit (out_host: a host array of n floats): the trainer's random times, drawn
 * without a device round trip.  FBSMI_ERR_ARG for n < 0 or a null array with n > 0. */
int fbsmi_uniform_host(uint32_t k0, uint32_t k1, int64_t n, float* out_host);

/* Row b of xt (B, D) = F[b] * x0[e] + sq[b] * xi[e]  (two products, one sum), x0 = row idx[b] of data (row b when idx is
 * NULL; the entries of idx must be valid rows of data, they are not checked) and xi = element e of normal(keys[b], (D,)),
 * drawn in the kernel: the batch gather, the draw and simulate_cond_forward(keep_path=False) in one pass, no (B, D) copy of
 * the batch and no noise array.  F, sq (B) float32, keys (B, 2) device arrays.  out_dtype 0: xt float32; 1: bfloat16.
 * Up to 64 workgroups per row.  When D is a multiple of 8 and data, xt are 16-byte aligned a thread owns four consecutive
 * elements in each half of the row (the two words of four cipher calls): 16-byte loads of data, 16-byte stores of a float32
 * xt, 8-byte stores of a bfloat16 xt; element-wise otherwise.  The kernel is bound by the cipher and the normal transform.
 * FBSMI_ERR_ARG for a null pointer (but idx), B < 1, D < 1, D > 2^32 - 4, out_dtype outside {0, 1}, or more workgroups than
 * one grid holds. */
int fbsmi_dsm_noise_batched(const float* data, const int32_t* idx, const uint32_t* keys, const float* F, const float* sq,
                            int64_t B, int64_t D, int out_dtype, void* xt, void* stream);

/* The loss mean_b(mean_e((net - cond_score)^2) Q_b) and its derivative with respect to net, in one pass over net (B, D;
 * net_dtype 0 float32, 1 bfloat16).  With cond_score = -(xt - F x0) / Q and sq = sqrt(Q) the summand is r^2 with
 *     r = sq[b] * net[b][e] + e_be,
 *   mode 0 (drawn):  e_be = element e of normal(keys[b], (D,)), exactly the xi of fbsmi_dsm_noise_batched; xt, data, idx
 *                    and F are not read;
 *   mode 1 (stored): e_be = (xt[b][e] - F[b] * x0[e]) / sq[b], a correctly rounded quotient, from a float32 xt (B, D) and
 *                    x0 = row idx[b] of data (row b when idx is NULL); keys is not read.  The path layout needs this form:
 *                    its points are sums of several draws.  The difference xt - F x0 cancels for small times: below
 *                    t ~ 0.02 its rounding error alone exceeds 1e-5 relative in the loss, in the reference's own
 *                    float32 evaluation as much as here.
 *   S_b = tree_sum_e(r^2) -> row_sums[b] (row_sums may be NULL);   loss[0] = inv * tree_sum_b(S_b), inv = float32(1 / (B D))
 *   from the host;   dnet[b][e] = gc[b] * r in net's dtype, gc[b] = float32(2 sq[b] / (B D)) from the host.
 * S_b and row b of dnet depend on row b alone: they have the same bits for any B and any position of the row.
 * Two launches: aligned chunks of 2048 elements of a row, spread over up to 64 workgroups per row, write dnet and their
 * subtree roots into workspace (fbsmi_dsm_loss_workspace_bytes(B, D) bytes; 0 for a refused shape); one workgroup finishes
 * the trees.  16-byte accesses when D is a multiple of 8 and the arrays are 16-byte aligned, element-wise otherwise.
 * FBSMI_ERR_ARG for a null pointer the mode reads or writes, B < 1, D < 1, D > 2^32 - 4, net_dtype or mode outside {0, 1},
 * or more workgroups than one grid holds. */
size_t fbsmi_dsm_loss_workspace_bytes(int64_t B, int64_t D);
int fbsmi_dsm_loss_batched(const void* net, int net_dtype, int mode, const uint32_t* keys, const float* xt, const float* data,
                           const int32_t* idx, const float* F, const float* sq, const float* gc, float inv, int64_t B,
                           int64_t D, void* dnet, float* row_sums, float* loss, void* workspace, void* stream);

/* out[0] = tree_sum_i(x[i] * x[i]) of a flat float32 vector, in one pass over it (squaring through fbsmi_math_map and
 * fbsmi_sum would be two, and a vector of scratch).  workspace: fbsmi_sqnorm_workspace_bytes(n) bytes.
 * FBSMI_ERR_ARG for a null pointer or n < 1. */
size_t fbsmi_sqnorm_workspace_bytes(int64_t n);
int fbsmi_sqnorm(const float* x, int64_t n, float* out, void* workspace, void* stream);

/* optax.chain(clip_by_global_norm(max_norm), adam(lr, b1, b2, eps)) and the reference's ema_kernel in one pass over the flat
 * float32 vectors p, g, m, v, ema (n); g is read only.
 *     s = 1 if gnorm2 is NULL or sqrt(gnorm2[0]) < max_norm, else max_norm / sqrt(gnorm2[0])   (gnorm2: a device scalar)
 *     g' = g * s;   m = b1 * m + (1 - b1) * g';   v = b2 * v + (1 - b2) * (g' * g')
 *     u = (m / bc1) / (sqrt(v / bc2) + eps);   p = p - lr * u
 *     ema_mode 0: ema untouched (it may be NULL);  1: ema = p;  2: ema = decay * ema + (1 - decay) * p   (the new p)
 * 1 - b1, 1 - b2 and 1 - decay are float32 differences; lr, bc1 = 1 - b1^t and bc2 = 1 - b2^t are float32 values the host
 * computed in float64 and rounded once.  sqrt and the quotients are correctly rounded.
 * FBSMI_ERR_ARG for a null pointer, n < 1, ema_mode outside {0, 1, 2}, bc1 or bc2 not positive, or max_norm not positive
 * with gnorm2 given. */
int fbsmi_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float b1, float b2,
                        float eps, float bc1, float bc2, const float* gnorm2, float max_norm, int ema_mode, float decay,
                        void* stream);

/* HIP-event timing hooks: average duration in microseconds of the propagate ("Euler") kernel
 * over the launches since the last reset; 0 launches -> returns 0. Only measured when
 * fbsmi_lg_sweep_profile(s, 1) was set (events force non-graph launches). */
int fbsmi_lg_sweep_profile(fbsmi_lg_sweep* s, int enable);
int fbsmi_lg_sweep_kernel_us(fbsmi_lg_sweep* s, int which, double* avg_us, int64_t* launches);

#ifdef __cplusplus
}
#endif

#endif /* FBSMI_H */
