"""CPU: the restatement of the image twisted-SMC step kernels (tests/tw_img_restate.py) differentiates the twisting function
the way float64 autograd does on the reference formulation, and the host key schedule of make_image_twisted_batched equals
the nested splits of conditional_sampler / twisted_smc."""
import math

import numpy as np
import torch

from tw_img_restate import TwStep, step_scalars


def _role(rng, D, dv):
    """A scattered mask: dv of the D image positions observed, in a shuffled order."""
    role = np.empty(D, np.int64)
    pos = rng.permutation(D)
    role[pos[:dv]] = ~np.arange(dv)
    role[pos[dv:]] = np.arange(D - dv)
    return role


def test_restated_gradient_equals_float64_autograd_on_the_reference_formulation():
    """inpainting_twisted.py:97-126 as restated in fbs_amd/twisted.py::_twist, in float64 torch: den = uv + rd dt, the masked
    Gaussian log-density of y at den, summed; its gradient with respect to uv goes through the coupling score
    s(x, t) = -c x + g * mean over the image's own pixels.  The restatement's closed form takes the network's part as the
    vector-Jacobian product -c ct + g mean(ct) of its own cotangent."""
    from fbs_amd.sdes import StationaryLinLinearSDE
    rng = np.random.default_rng(3)
    sde = StationaryLinLinearSDE(beta_min=0.02, beta_max=5.0, t0=0.0, T=2.0)
    ts = np.linspace(0, 2.0, 7)
    c, gc = 0.6, 0.8
    for (n, D, dv), k in (((5, 81, 65), 1), ((4, 288, 238), 3), ((3, 400, 375), 6)):
        cx, cs, dt, sd, var_y = step_scalars(sde, ts, k)
        role = _role(rng, D, dv)
        st = TwStep(role, cx, cs, dt, sd, var_y)
        X, y = rng.normal(size=(n, D)), rng.normal(size=dv)
        S = -c * X + gc * X.mean(1, keepdims=True)
        ct, _ = st.cotangent(X, S, y)
        V = -c * ct + gc * ct.mean(1, keepdims=True)
        got, _ = st.grad(X, S, V, y)
        # the reference formulation under autograd
        x = torch.tensor(X, dtype=torch.float64, requires_grad=True)
        yfull, m = torch.zeros(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
        obs = np.nonzero(role < 0)[0]
        yfull[obs] = torch.tensor(y[~role[obs]])
        m[obs] = 1.0
        score = -c * x + gc * x.mean(1, keepdim=True)
        den = x + (cx * x + cs * score) * dt
        scale = math.sqrt(var_y)
        z = (yfull - den) / scale
        lp = ((-0.5 * z * z - math.log(scale) - 0.5 * math.log(2.0 * math.pi)) * m).sum()
        want = torch.autograd.grad(lp, x)[0].numpy()
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (n, D, np.abs(got - want).max())
        # and the twisting log-density itself
        lp_rows, _ = st.twist(X, S, y)
        np.testing.assert_allclose(lp_rows.sum(), float(lp.detach()), rtol=1e-12)


def test_key_schedule_equals_the_nested_splits():
    """conditional_sampler: (filter, select) = split(key); twisted_smc: (init, scan) = split(filter, 2), split(scan, nsteps),
    (resampling_k, prop_k) = split(keys_k, 2)."""
    from fbs_amd import ops
    from fbs_amd.twisted import twisted_filter_key_schedule, twisted_key_schedule
    T = 5
    for B in (1, 3):
        keys = ops.split(ops.PRNGKey(2026), B)
        ks = twisted_key_schedule(keys, T)
        assert all(ks[n].shape == (B, 2) for n in ("filter", "select", "init"))
        assert all(ks[n].shape == (T, B, 2) for n in ("resampling", "prop"))
        assert all(a.dtype == np.uint32 for a in ks.values())
        for b in range(B):
            key_filter, key_select = ops.split(keys[b])
            key_init, key_scan = ops.split(key_filter, 2)
            np.testing.assert_array_equal(ks["filter"][b], key_filter)
            np.testing.assert_array_equal(ks["select"][b], key_select)
            np.testing.assert_array_equal(ks["init"][b], key_init)
            for k, key_k in enumerate(ops.split(key_scan, T)):
                key_resampling, key_prop = ops.split(key_k, 2)
                np.testing.assert_array_equal(ks["resampling"][k, b], key_resampling)
                np.testing.assert_array_equal(ks["prop"][k, b], key_prop)
        sub = twisted_filter_key_schedule(ks["filter"], T)
        for name in ("init", "resampling", "prop"):
            np.testing.assert_array_equal(sub[name], ks[name])
        assert len({tuple(r) for r in np.concatenate([ks["resampling"], ks["prop"]]).reshape(-1, 2)}) == 2 * B * T
