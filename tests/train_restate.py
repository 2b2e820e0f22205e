"""Restatements for the score-matching trainer (fbs_amd/csrc/fbsmi_train.hip, fbs_amd/sdes/losses.py, fbs_amd/train.py).

Two families, both plain numpy:
  * float32 restatements of each kernel's specification in include/fbsmi.h, one rounded operation per line, built on
    oracle.normal / oracle.split / oracle.tree_sum: the kernels must equal them bit for bit;
  * float64 restatements of the reference's own formulas (fbs/sdes/linear.py cond_score_t_0 and the Q weighting, optax's
    adam, clip_by_global_norm and schedules, fbs/nn/utils.py ema_kernel) on the same float32 inputs: the kernels must be
    within the project's float32 criterion, 1e-5 relative, of them.
Each float64 restatement takes a `mistake` argument that plants one of the obvious errors, for the test that shows the
restatement would tell it apart.
"""
import functools
import math

import numpy as np

import oracle as O

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# float32: the kernels' specifications
# ------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the float32 value of its bfloat16 rounding (to nearest even)."""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(f32).reshape(np.shape(x))


def bf16_round_full(x):
    """bf16_round on all of float32: to nearest even, overflow to infinity, and any NaN in gives a NaN out (bf16_round adds
    the rounding increment to a NaN's payload too, which carries 0x7fffffff over into -0)."""
    x = np.ascontiguousarray(x, f32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16) & 0xffffffff
    quiet = ((u >> 16) | 0x40) << 16                       # the kernel's choice; only "is a NaN" is specified
    r = np.where((u & 0x7fffffff) > 0x7f800000, quiet, r)
    return r.astype(np.uint32).view(f32).reshape(np.shape(x))


def noise_f32(data, idx, keys, F, sq):
    """fbsmi_dsm_noise_batched: (xt (B, D) float32, xi (B, D))."""
    B, D = len(keys), data.shape[1]
    xt, xi = np.zeros((B, D), f32), np.zeros((B, D), f32)
    for b in range(B):
        x0 = data[b if idx is None else idx[b]]
        xi[b] = O.normal(keys[b], (D,))
        xt[b] = f32(F[b]) * x0 + f32(sq[b]) * xi[b]
    return xt, xi


def loss_f32(net, e, sq, gc, inv):
    """fbsmi_dsm_loss_batched after its noise form e (B, D) is known: (S (B,), loss, dnet (B, D) float32)."""
    B = net.shape[0]
    S, dnet = np.zeros(B, f32), np.zeros_like(net, dtype=f32)
    for b in range(B):
        r = f32(sq[b]) * net[b] + e[b]
        S[b] = O.tree_sum(r * r)
        dnet[b] = f32(gc[b]) * r
    return S, f32(inv) * O.tree_sum(S), dnet


def stored_noise_f32(xt, data, idx, F, sq):
    """mode 1: e = (xt - F x0) / sq, the quotient correctly rounded."""
    e = np.zeros_like(xt)
    for b in range(xt.shape[0]):
        x0 = data[b if idx is None else idx[b]]
        e[b] = (xt[b] - f32(F[b]) * x0) / f32(sq[b])
    return e


# ------------------------------------------------------------------------------------------------
# float64: the reference's formulas
# ------------------------------------------------------------------------------------------------
def cond_score_t_0(x, F, Q, x0):
    """fbs/sdes/linear.py:186-188."""
    return -(x - F * x0) / Q


def loss_f64(net, xt, x0, F, sq, mistake=None):
    """linear.py:338-340: mean_b(mean_e((net - cond_score)^2) Q_b), Q = sq^2; all arguments widened to float64.
    net, xt, x0 (B, D); F, sq (B,).  mistakes: 'no_q' drops the weight, 'sq_for_q' weights by sqrt(Q)."""
    net, xt, x0, F, sq = (np.asarray(a, np.float64) for a in (net, xt, x0, F, sq))
    Q = sq * sq
    cs = cond_score_t_0(xt, F[:, None], Q[:, None], x0)
    per_row = np.mean((net - cs) ** 2, axis=1)
    w = {None: Q, 'no_q': np.ones_like(Q), 'sq_for_q': sq}[mistake]
    return float(np.mean(per_row * w))


def clip_by_global_norm_f64(g, max_norm, mistake=None, gnorm2=None):
    """optax.clip_by_global_norm.  mistake 'by_value' clips every entry to [-max_norm, max_norm].  gnorm2: the squared norm
    when it is given and not g's own (fbsmi_adam_ema_step reads it from a device scalar): 0 leaves g alone, inf gives
    zeros, and NaN makes every entry NaN, since where(norm < max_norm, g, ...) then takes the scaled branch."""
    g = np.asarray(g, np.float64)
    if mistake == 'by_value':
        return np.clip(g, -max_norm, max_norm)
    n = math.sqrt(float(np.sum(g * g)) if gnorm2 is None else float(gnorm2))
    return g if n < max_norm else g / n * max_norm


def adam_f64(p, g, m, v, lr, b1, b2, eps, count, mistake=None):
    """optax.adam at optax's count (0 at the first step): (p, m, v).  mistakes: 'eps_in_sqrt', 'count_from_1'."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    t = count + (2 if mistake == 'count_from_1' else 1)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mh, vh = m / (1 - b1 ** t), v / (1 - b2 ** t)
    u = mh / np.sqrt(vh + eps) if mistake == 'eps_in_sqrt' else mh / (np.sqrt(vh) + eps)
    return p - lr * u, m, v


def ema_mode_of(count, count_start, count_every):
    """fbs/nn/utils.py:71-81 as the ema_mode of fbsmi_adam_ema_step."""
    if count < count_start:
        return 1
    return 2 if count % count_every == 0 else 0


def ema_f64(ema, p, mode, decay):
    ema, p = np.asarray(ema, np.float64), np.asarray(p, np.float64)
    return (ema, p, decay * ema + (1 - decay) * p)[mode]


def cosine_f64(count, init, decay_steps, alpha):
    c = min(count, decay_steps) / decay_steps
    return init * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * c)) + alpha)


def exponential_f64(count, init, transition_steps, rate):
    return init if count <= 0 else init * rate ** (count / transition_steps)


def closed_form_run(steps=200, n=8, T=2.0, lr=0.05, a=-0.5, b=1.0, c=1.0, b1=0.9, b2=0.999, eps=1e-8):
    """The closed-form training run: nn = -(x - F theta) / Q against data = c, so loss = (theta - c)^2 mean(F^2 / Q) on the
    fixed save_mem grid.  Returns (theta, first loss, last loss) of `steps` adam steps from theta = 0, in float64."""
    ts = np.linspace(T / n, T, n)
    F, Q = np.exp(a * ts), b * b / (2 * a) * (np.exp(2 * a * ts) - 1)
    w = float(np.mean(F * F / Q))
    theta, m, v, losses = 0.0, 0.0, 0.0, []
    for k in range(steps):
        losses.append((theta - c) ** 2 * w)
        th, m, v = adam_f64(np.array([theta]), np.array([2 * (theta - c) * w]), m, v, lr, b1, b2, eps, k)
        theta, m, v = float(th[0]), m, v
    return theta, losses[0], (theta - c) ** 2 * w


# ------------------------------------------------------------------------------------------------
# shared inputs of the kernel tests: computed once per shape
# ------------------------------------------------------------------------------------------------
NDATA = 7
IDX = np.array([3, 0, 3, 6, 1], np.int32)          # permuted, with a repeat
TIMES = np.array([0.02, 0.3, 0.75, 1.4, 2.0])      # the fixed grid of the stored-point loss: t >= 0.02


def lin_tables(ts, count):
    """(F, sq, gc) float32 of the reference's default SDE (beta_min 0.02, beta_max 5, T 2) from t0 = 0."""
    ts = np.asarray(ts, np.float64)
    r = 0.02 * ts + 0.5 * ts * ts * (5.0 - 0.02) / 2.0
    F, sq = np.exp(-0.5 * r).astype(f32), np.sqrt(1 - np.exp(-r)).astype(f32)
    return F, sq, (2.0 * sq.astype(np.float64) / count).astype(f32)


def idx_of(B):
    """B rows of the NDATA data rows: IDX, then a seeded draw with repeats."""
    if B <= len(IDX):
        return IDX[:B]
    more = np.random.default_rng(4242).integers(0, NDATA, B - len(IDX)).astype(np.int32)
    return np.concatenate([IDX, more])


def times_of(B):
    """B times in [0.02, 2]: TIMES, then an even grid over the same interval."""
    if B <= len(TIMES):
        return TIMES[:B]
    return np.concatenate([TIMES, np.linspace(0.02, 2.0, B - len(TIMES))])


@functools.lru_cache(maxsize=None)
def case(D, B=5):
    """Inputs and float32 expectations for B rows of D elements: a dict of read-only arrays.  With more rows than data has
    (B > NDATA) only the gathered layout exists: "xt" is left out and "xi", which depends on the keys alone, stays."""
    rng = np.random.default_rng(1000 + D)
    data = rng.uniform(0, 1, (NDATA, D)).astype(f32)
    keys = O.split(O.PRNGKey(77 + D), B)
    F, sq, gc = lin_tables(times_of(B), B * D)
    inv = f32(1.0 / (B * D))
    net = rng.normal(size=(B, D)).astype(f32)
    net16 = bf16_round(net)
    idx = idx_of(B)
    out = dict(D=D, B=B, data=data, keys=keys, F=F, sq=sq, gc=gc, inv=inv, net=net, net16=net16, idx=idx)
    out["xt_idx"], out["xi_idx"] = noise_f32(data, idx, keys, F, sq)
    if B <= NDATA:
        out["xt"], out["xi"] = noise_f32(data, None, keys, F, sq)
    else:
        out["xi"] = out["xi_idx"]
    out["x0_idx"] = data[idx]
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
