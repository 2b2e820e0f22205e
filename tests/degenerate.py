"""Collapsed counterparts of the toys in helpers.py: strong u-v coupling and an outlier observation, so that the
weight vectors the in-kernel resamplers see have an effective sample size near 1, long runs of exactly-zero weights and a
kill fraction near 1 -- the opposite of the benign regime (ESS ~ N, no zero weight) the toys produce.
Not collected: the tests import it.  test_degenerate_inputs.py proves on the CPU that each input collapses."""
import numpy as np

from helpers import oracle_model_from

f32 = np.float32


def collapse_2d():
    """toy_2d with correlation 0.999999 between u and v and an observation at 1000 (prior standard deviation 0.7)."""
    return dict(m0=np.array([-1., 1.]), cov0=np.array([[2., .999999], [.999999, .5]]), y0=np.array([1000.], f32), du=1)


def _coupled(seed, du, H, m0, y0, noise):
    """cov(u) as in toy_4d / toy_31 (A A^T / 4 + I / 2 of the seeded A's leading block), v = H u + N(0, noise I)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(4, 4))
    cov_u = (A @ A.T / 4 + 0.5 * np.eye(4))[:du, :du]
    H = np.asarray(H, np.float64)
    cov0 = np.block([[cov_u, cov_u @ H.T], [H @ cov_u, H @ cov_u @ H.T + noise * np.eye(H.shape[0])]])
    return dict(m0=np.asarray(m0, np.float64), cov0=cov0, y0=np.asarray(y0, f32), du=du)


def collapse_4d():
    """Counterpart of toy_4d (du = dv = 2): v observes u with noise variance 1e-4; y0 far in the tail, opposite signs."""
    return _coupled(7, 2, np.eye(2), [0.5, -1., 1., 0.2], [3000., -4000.], 1e-4)


def collapse_31():
    """Counterpart of toy_31 (du = 3, dv = 1): v observes u_0 - u_1 + u_2 with noise variance 1e-4; outlier y0."""
    return _coupled(11, 3, np.array([[1., -1., 1.]]), [0.1, 0.2, -0.3, 1.], [7000.], 1e-4)


def collapse_gp(d, dv=None, noise=1e-2, y_scale=20, seed=5):
    """toy_gp's joint covariance with observation noise `noise` I instead of I, and y0 scaled by y_scale (the same
    seeded draw as toy_gp's)."""
    dv = d if dv is None else dv
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    H = np.eye(d)[:dv]
    joint = np.block([[cov, cov @ H.T], [H @ cov, H @ cov @ H.T + noise * np.eye(dv)]])
    rng = np.random.default_rng(seed)
    return dict(m0=np.zeros(d + dv), cov0=joint, y0=(y_scale * rng.normal(size=dv)).astype(f32), du=d)


def cpu_bridge(toy, T, Tend=1.0):
    """The product's bridge on the CPU device (host tables only, nothing is launched), const SDE (-0.5, 1)."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    return fbs_amd.LinearGaussianBridge(toy["m0"], toy["cov0"], StationaryConstLinearSDE(a=-0.5, b=1.),
                                        np.linspace(0, Tend, T + 1), toy["du"], device="cpu")


def sweep_inputs(toy, N, T, seed=None):
    """x0 and bs_star of the sweep tests (test_fused_sweep_matches_oracle's recipe)."""
    rng = np.random.default_rng(N + T if seed is None else seed)
    return rng.normal(size=toy["du"]).astype(f32), rng.integers(0, N, T + 1).astype(np.int32)


def profile_of(O, log_wss):
    """(ess, zero_frac, kill_frac), one entry per row of stored log-weights.  A weight is zero when oracle.exp of its
    log-weight is exactly 0.0f -- what the resampling kernels are handed."""
    ess, zero, kill = [], [], []
    for lw in np.asarray(log_wss, f32):
        w32 = O.exp(lw)
        w = w32.astype(np.float64)
        ess.append(w.sum() ** 2 / (w * w).sum())
        zero.append(float(np.mean(w32 == 0.0)))
        kill.append(1.0 - w.mean() / w.max())
    return np.array(ess), np.array(zero), np.array(kill)


def forward_log_wss(O, om, key, x0, y0, bs, N, eb=True, ef=False):
    """The stored log-weights (T + 1, n) of the conditional SMC pass inside oracle.gibbs_kernel_lg(om, key, x0, y0, bs, N,
    eb, ef): the same key splits and initial particles (gibbs.py:126-148)."""
    k_fwd, k_csmc, _ = O.split(key, 3)
    path = O.lg_fwd_sampler(om, k_fwd, np.concatenate([np.asarray(x0, f32).reshape(-1), np.asarray(y0, f32).reshape(-1)]))
    us, vs = path[::-1, :om.du].copy(), path[::-1, om.du:].copy()
    k_pass = O.split(k_csmc, 4 if eb else 2)[0]
    if ef:
        us0 = O.normal(O.split(k_pass, 2)[0], (N + 1, om.du))
        us0[bs[0]] = us[0]
        lw0 = O.lg_likelihood_logpdf(om, 0, vs[0], us0, vs[1])
    else:
        us0 = np.tile(us[0], (N, 1)).astype(f32)
        lw0 = np.full(N, f32(-np.log(N)), f32)
    return O.csmc_forward_pass_lg(om, k_pass, us, bs, vs, us0, lw0, store=True)["log_wss"]


def weight_profile(O, model, N, T, Tend=1.0, key=None, x0=None, bs=None, eb=True, ef=False):
    """Per-step (ess, zero_frac, kill_frac) of the weights a Gibbs sweep of `model` (a toy dict) meets with N particles on
    linspace(0, Tend, T + 1): rows 0 .. T - 1 are what the killing resampler is handed, row T what force_move is."""
    om = oracle_model_from(O, cpu_bridge(model, T, Tend))
    dx0, dbs = sweep_inputs(model, N, T)
    key = O.split(O.PRNGKey(42), 2)[1] if key is None else key
    lws = forward_log_wss(O, om, key, dx0 if x0 is None else x0, model["y0"], dbs if bs is None else bs, N, eb, ef)
    return profile_of(O, lws)


# ---- the cases of tests/test_gpu_degenerate.py, proven collapsed on the CPU by tests/test_degenerate_inputs.py -------------
TOYS = {"2d": collapse_2d, "4d": collapse_4d, "31": collapse_31}
GP = dict(noise=1e-4, y_scale=1000)   # the wide cases: at the defaults no resampled step of these sweeps reaches zero_frac 0.9

# (id, toy, N, T, Tend, explicit_backward, explicit_final, forcing switches, the step kernel the dispatch code reaches)
NARROW = [
    ("one-launch-10", "2d", 10, 12, 0.5, True, False, {}, "k_lg_sweep1"),
    ("one-launch-256", "4d", 256, 6, 1.0, True, False, {}, "k_lg_sweep1"),
    ("prop1-777", "31", 777, 6, 1.0, True, False, {}, "k_lg_prop1"),
    ("prop1t-512", "2d", 512, 6, 0.5, True, False, {}, "k_lg_prop1t<., 1>"),
    ("prop1t-511-ef", "2d", 511, 6, 0.5, True, True, {}, "k_lg_prop1t<., 1>, 512 slots"),
    ("prop1t-512-ef", "4d", 512, 6, 1.0, True, True, {}, "k_lg_prop1t<., 1>, 2^k + 1 slots"),
    ("prop1th-2048", "2d", 2048, 6, 0.5, True, False, {"FBSMI_TREE_HALVES": "2"}, "k_lg_prop1th<., 2>"),
    ("prop1tp-2048", "2d", 2048, 6, 0.5, True, False, {"FBSMI_TREE_HALVES": "2", "FBSMI_PROP_HALFWAVE": "0"}, "k_lg_prop1tp<., 2>"),
    ("four-tiles-2048", "31", 2048, 6, 1.0, True, False, {"FBSMI_TREE_HALVES": "4"}, "k_lg_prop1th<., 4>"),
    ("prop2t-1024", "2d", 1024, 6, 0.5, True, False, {"FBSMI_TWO_SLOT_PROP": "1"}, "k_lg_prop2t"),
    ("prop2-1024", "2d", 1024, 6, 0.5, True, False, {"FBSMI_TWO_SLOT_PROP": "1", "FBSMI_TREE_STEP": "0"}, "k_lg_prop2"),
    ("stored-512", "31", 512, 6, 1.0, False, False, {}, "k_lg_prop1t<., 1>, stored path"),
]
PROPQ4 = ("propQ4-200000", "2d", 200000, 3, 2.0, True, False, {}, "k_lg_heaps + k_lg_propQ<4>")
PROPQ16 = ("propQ16-1100000", "2d", 1100000, 3, 2.0, True, False, {}, "k_lg_heaps + k_lg_propQ<16>")
# three chains of collapse_2d in one launch sequence, (N, T, Tend) and the chains' x0: at the prior mean, at E[x0 | y0],
# and five prior standard deviations out
CHAINS = ("chains-512", "2d", 512, 6, 0.5, (-1.0, 1996.998, 7.0))
# (id, du, dv, N, C, T, Tend, regime)
WIDE = [
    ("one-tile-40", 20, 20, 40, 1, 6, 0.5, "k_lgw_gemm<1>"),
    ("tiled-300", 20, 20, 300, 1, 6, 0.5, "k_lgw_anc + k_lgw_gemm<0>"),
    ("odd-300", 33, 17, 300, 1, 6, 0.5, "k_lgw_anc + k_lgw_gemm<0>, D = 50"),
    ("fat-5632", 20, 20, 5632, 3, 6, 0.5, "k_lgw_anc + k_lgw_gemm_fat<true>"),
]
# the fused filters: (model, n); every model on linspace(0, 1, 9)
FILTERS = [("2d", 64), ("2d", 256), ("2d", 257), ("2d", 512), ("2d", 70000), ("gp20", 200), ("gp20", 1000)]
FILTER_T = 8
# twisted SMC: (d, T, N)
TW_SHAPES = [(3, 8, 100), (3, 8, 256), (10, 6, 257), (24, 6, 1000)]


def named_toy(name):
    if name in TOYS:
        return TOYS[name]()
    assert name.startswith("gp")
    d, _, dv = name[2:].partition("v")
    return collapse_gp(int(d), int(dv) if dv else None, **GP)


def sweep_key(O, trial=0):
    return O.split(O.PRNGKey(42 + trial), 2)[1]


def filter_inputs(O, om, y0, n, nchains=3):
    """Adversarial inputs of the fused filters: vs the reversed oracle forward path of the collapsed model, initial
    particles five standard deviations wide.  -> keys (C, 2), vs (C, T + 1, dv), init (C, n, du)."""
    keys, vs, init = [], [], []
    for kc in O.split(O.PRNGKey(3), nchains):
        k1, k2, k3 = O.split(kc, 3)
        vs.append(O.lg_fwd_sampler(om, k1, np.asarray(y0, f32))[::-1].copy())
        init.append((f32(5) * O.normal(k2, (n, om.du))).astype(f32))
        keys.append(k3)
    return np.stack(keys), np.stack(vs), np.stack(init)


def filter_weight_profile(O, om, key, vs, init, resampling):
    """(ess, zero_frac, kill_frac) of the weights the filter's resampler is handed at each step: the stored filtering
    particles of oracle.bootstrap_filter_lg, re-weighted as smc.py:42-47 does."""
    filt, _ = O.bootstrap_filter_lg(om, key, vs, init, resampling, return_last=False)
    lws = [O.normalise(O.lg_likelihood_logpdf(om, k, vs[k + 1], filt[k], vs[k]), True) for k in range(om.T)]
    return profile_of(O, np.stack(lws))


def collapse_tw(d, T, device):
    """The GaussianTwisted of test_gpu_tw_fused._model (const SDE) with obs_var = 0.01 and y scaled by 20."""
    import fbs_amd
    from fbs_amd.sdes import StationaryConstLinearSDE
    zs = np.linspace(0., 5., d)
    cov = np.exp(-np.abs(zs[None, :] - zs[:, None]))
    rng = np.random.default_rng(100 + d)
    mean, y = 0.3 * rng.normal(size=d), (20 * rng.normal(size=d)).astype(f32)
    return fbs_amd.GaussianTwisted(mean, cov, StationaryConstLinearSDE(a=-0.5, b=1.), np.linspace(0., 1., T + 1), 0.01, y,
                                   device=device)


def tw_run_recording(O, restate, key, N, resampling):
    """Restate.run plus the weight vectors its resampler was handed -> ((xs, lws, ancestors), [weights per step])."""
    seen = []
    real = getattr(O, resampling)

    def recording(w, k):
        seen.append(np.array(w, f32))
        return real(w, k)

    xs, lws, inds = O.twisted_smc_np(np.asarray(key, np.uint32), restate.y, restate.ts, restate.init_sampler,
                                     restate.transition_logpdf, restate.twisting_logpdf, restate.twisting_prop_sampler,
                                     restate.twisting_prop_logpdf, recording, N)
    return (xs, lws, np.stack(inds).astype(np.int32)), seen


def profile_of_weights(ws):
    """profile_of for weight vectors (not log-weights)."""
    ess, zero, kill = [], [], []
    for w32 in ws:
        w = np.asarray(w32, np.float64)
        ess.append(w.sum() ** 2 / (w * w).sum())
        zero.append(float(np.mean(np.asarray(w32) == 0.0)))
        kill.append(1.0 - w.mean() / w.max())
    return np.array(ess), np.array(zero), np.array(kill)


# ---- pMCMC: one iteration of two chains; the oracle accepts from log_ell = -3e38 and rejects from log_ell = 0 ---------------
PMCMC = [("2d", 64), ("gp20", 200)]
PMCMC_T = 8


def ref_sampler_of(O, toy, br):
    """As test_gpu_pmcmc_fused._ref_sampler: oracle.lg_ref_sampler at du = dv = 1, the order include/fbsmi.h fixes otherwise."""
    import fsamp_restate
    from fbs_amd.sdes.linear import discretise_linear_sde_np
    if br.du == 1 and br.dv == 1:
        FQ_T = discretise_linear_sde_np(br.sde, br.ts_np[-1], br.ts_np[0])
        return lambda k, yT, n: O.lg_ref_sampler(toy["m0"], toy["cov0"], FQ_T, 1, k, yT, n)
    tab = br.pmcmc_tables_host(None)
    return lambda k, yT, n: fsamp_restate.ref_restated(O, tab, k, yT, n)


def pmcmc_inputs(O, om, toy, br):
    """-> keys (2, 2), uT (2, du), log_ell (2,), ys (2, T + 1, dv), mean_path (T + 1, dv)"""
    ts = br.ts_np
    mean_path = (np.asarray(br.sde.mean(ts, ts[0], 1.0), f32).reshape(-1, 1) * toy["y0"].reshape(1, -1)).astype(f32)
    uT = np.stack([np.full(br.du, u, f32) for u in (0.3, -0.7)])
    ys = np.stack([O.lg_fwd_sampler(om, O.PRNGKey(1 + c), toy["y0"]) for c in range(2)])
    return O.split(O.PRNGKey(21), 2), uT, np.array([-3e38, 0.0], f32), ys, mean_path


def pmcmc_oracle_iteration(O, om, key, uT, log_ell, ys, y0, n, ref, mean_path, delta):
    """oracle.pmcmc_kernel_lg plus the two MCMCState fields it does not return, from the same primitives (as
    test_gpu_pmcmc_fused._oracle_iteration): -> (uT, log_ell, ys, is_accepted, acceptance_prob, prop_log_ell)."""
    want = O.pmcmc_kernel_lg(om, key, uT, log_ell, ys, y0, n, ref, mean_path, delta)
    k_prop, k_u0, k_f, _ = O.split(key, 4)
    fwd = lambda k: O.lg_fwd_sampler(om, k, y0)
    prop_ys = fwd(k_prop) if delta is None else O.pcn_proposal(k_prop, delta, np.asarray(ys, f32), mean_path, fwd)
    vs = prop_ys[::-1].copy()
    _, prop_ell = O.pmcmc_filter_step_lg(om, k_f, vs, ref(k_u0, vs[0], n), "stratified")
    prob = O.exp(np.array([np.minimum(f32(0.0), f32(prop_ell) - f32(log_ell))], f32))[0]
    return want + (prob, f32(prop_ell))
