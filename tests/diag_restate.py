"""The diagnostic rows (lse, ess) of the fused engines (include/fbsmi.h, fbsmi_lg_sweep_set_diagnostics), rebuilt on the CPU
from oracle pieces only: the unnormalised log-weight vector of every step, then oracle.logsumexp / oracle.ess of it.
Not collected: the tests import it.  tests/test_diag_restate.py proves the reconstruction before tests/test_gpu_diag.py
uses it as the yardstick."""
import numpy as np

f32 = np.float32


def rows_of(O, lws):
    """(lse, ess), one entry per vector of unnormalised log-weights."""
    lws = [np.asarray(lw, f32) for lw in lws]
    return np.array([O.logsumexp(lw) for lw in lws], f32), np.array([O.ess(lw) for lw in lws], f32)


# ---- Gibbs sweep -----------------------------------------------------------------------------------------------------------
def sweep_inputs_of(O, om, key, x0, y0, bs, N, eb=True, ef=False):
    """What oracle.gibbs_kernel_lg(om, key, x0, y0, bs, N, eb, ef) hands its conditional SMC pass (gibbs.py:126-148):
    -> (k_pass, us_star (T+1, du), vs (T+1, dv), us0 (n, du), lw0 (n)); with explicit_final lw0 is the init likelihood on the
    pinned initial particles (csmc.py:152-154)."""
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
    return k_pass, us, vs, us0, lw0


def sweep_lws_from_pass(O, om, vs, lw0, fwd):
    """The T + 1 unnormalised vectors of a stored pass `fwd` (oracle.csmc_forward_pass_lg(..., store=True)): row 0 the
    initial log-weights, row k the likelihood_logpdf values of step k - 1 on the resampled particles (csmc.py:140,145)."""
    lws = [np.asarray(lw0, f32)]
    for k in range(1, om.T + 1):
        lws.append(O.lg_likelihood_logpdf(om, k - 1, vs[k], fwd["uss"][k - 1][fwd["As"][k - 1]], vs[k - 1]))
    return lws


def sweep_lws(O, om, key, x0, y0, bs, N, eb=True, ef=False):
    """-> (the T + 1 unnormalised vectors of the sweep, the oracle's stored normalised log_wss (T + 1, n))."""
    k_pass, us, vs, us0, lw0 = sweep_inputs_of(O, om, key, x0, y0, bs, N, eb, ef)
    fwd = O.csmc_forward_pass_lg(om, k_pass, us, bs, vs, us0, lw0, store=True)
    return sweep_lws_from_pass(O, om, vs, lw0, fwd), fwd["log_wss"]


def sweep_rows_on(O, om, k_pass, us, vs, bs, N):
    """(lse, ess) of the pass with key k_pass on a given reference path `us` and observation path `vs` (explicit_final off):
    for the sweeps whose paths come from elsewhere (marg_y: the Doob bridge; the Schrodinger-bridge toy: Euler-Maruyama)."""
    us0 = np.tile(np.asarray(us, f32)[0], (N, 1)).astype(f32)
    lw0 = np.full(N, f32(-np.log(N)), f32)
    fwd = O.csmc_forward_pass_lg(om, k_pass, us, bs, vs, us0, lw0, store=True)
    return rows_of(O, sweep_lws_from_pass(O, om, vs, lw0, fwd))


def sweep_rows(O, om, key, x0, y0, bs, N, eb=True, ef=False):
    """(lse (T + 1), ess (T + 1)) of one sweep."""
    return rows_of(O, sweep_lws(O, om, key, x0, y0, bs, N, eb, ef)[0])


# ---- filters ---------------------------------------------------------------------------------------------------------------
def bootstrap_lws(O, om, key, vs, init, resampling):
    """Flow 0: -> (the T vectors log_weights of smc.py:65, the oracle's negative log-likelihood)."""
    filt, nell = O.bootstrap_filter_lg(om, key, vs, init, resampling, return_last=False)
    return [O.lg_likelihood_logpdf(om, k, vs[k + 1], filt[k], vs[k]) for k in range(om.T)], nell


def nell_from_lse(lse, n):
    """orc_bootstrap_filter_lg's accumulator (smc.py:67), sequentially in float32: log_nell -= c - log(n)."""
    logn, acc = f32(np.log(np.float64(n))), f32(0.0)
    for c in np.asarray(lse, f32):
        acc = f32(acc - f32(c - logn))
    return acc


def pmcmc_restated(O, om, key, vs, u0s, resampling):
    """Flow 1: pmcmc_filter_step (smc.py:138-152) on oracle pieces -> (the T vectors log_ws of :144, uT, log_ell)."""
    resample = {"stratified": O.stratified, "systematic": O.systematic}[resampling]
    vs = np.asarray(vs, f32).reshape(om.T + 1, om.dv)
    us = np.asarray(u0s, f32).reshape(-1, om.du).copy()
    logn, log_ell = f32(np.log(np.float64(us.shape[0]))), f32(0.0)
    lws = []
    for k, kk in enumerate(O.split(key, om.T)):                                  # :154
        k_prop, k_res = O.split(kk, 2)                                           # :142
        lw = O.lg_likelihood_logpdf(om, k, vs[k + 1], us, vs[k])                 # :144
        c = O.logsumexp(lw)                                                      # :145
        log_ell = f32(f32(log_ell - logn) + c)                                   # :146
        w = O.exp((lw - c).astype(f32))                                          # :147-148
        us = O.lg_transition_sampler(om, k, us[resample(w, k_res)], vs[k], k_prop)   # :149-150
        lws.append(lw)
    return lws, us, log_ell
