"""A numpy float32 restatement of the one-wave search for J of the two-launch Gibbs step (wave_tree_J in fbsmi_lg.hip),
written as the kernel does it: 256 leaves of a tree held four per lane by 64 lanes, levels 0-1 inside a lane, levels 2-7 as
butterfly records, nodes evaluated only along the walk (read from the lane that holds the midpoint), the path of the tile of
i* patched by folding the new leaf over that leaf's sibling sums, and the last two levels taken from the four leaves of one
lane.  N is a power of two with 2..256 tiles of 256 slots.

Every arithmetic step is a float32 operation on float32 operands (numpy scalars and arrays of dtype float32 only), in the
kernel's order, so the result is the kernel's J bit for bit -- and the oracle's, if the algorithm is right.

Also here: the oracle's own J of every step of a sweep, for the tests that compare with it."""
import numpy as np

F = np.float32
K_BLOCK = 256
LANES = np.arange(64)


def _up_sweep(x4):
    """x4: (64, 4) float32, the leaves of lane l at x4[l].  Returns the records of the up-sweep: the leaves, the sums of
    level 0, for each of the six butterfly levels the sum of the sibling block (ls[k][l]), and the root."""
    x4 = np.ascontiguousarray(x4, F)
    s01, s23 = x4[:, 0] + x4[:, 1], x4[:, 2] + x4[:, 3]
    s = s01 + s23
    ls = []
    for k in range(6):
        o = s[LANES ^ (1 << k)]                      # any lane of the sibling block holds its sum
        ls.append(o)
        s = np.where((LANES >> k) & 1, o + s, s + o)  # left + right
    assert s.dtype == F
    return dict(x=x4, s01=s01, s23=s23, ls=ls, root=s[0])


def _jprob(w, w_max, inv_n):
    return (F(1) - w / w_max) * inv_n


def _fold(x, sib, levels=8):
    for lv in range(levels):
        x = x + sib[lv]
    return x


def _sibling_sums(t, leaf):
    """The eight sibling sums of leaf `leaf` (0..255) on its path to the root, leaf level first, read from the records of
    the lane that holds it."""
    l, pos = leaf >> 2, leaf & 3
    x = t["x"][l]
    return [x[pos ^ 1], (t["s01"] if pos & 2 else t["s23"])[l]] + [t["ls"][k][l] for k in range(6)]


def _half(t, lo, c):
    """Sum of the left half of node [lo, lo + 2^(c+1)), from the lane of the node's midpoint."""
    ml = (lo + (1 << c)) >> 2
    if c >= 2:
        return t["ls"][c - 2][ml]
    if c == 1:
        return t["s01"][ml]
    return t["x"][ml][2 if lo & 2 else 0]


def _mid(y4, lo, c):
    """The value y of the leaf at the midpoint of that node."""
    mid = lo + (1 << c)
    return y4[mid >> 2][mid & 3]


class _Walk:
    def __init__(self, q, E):
        self.q, self.P, self.E = q, F(0), E

    def left(self, s, y):   # tree_walk
        t = self.P + s
        gl = bool(self.q <= t + y)
        if gl:
            self.E = t
        else:
            self.P = t
        return gl


def restate_J(w, i_ref, u3, N):
    """J = choice(key_3, N, (), p=J_prob) of the conditional killing resampler for normalised weights w (float32, N of
    them), reference index i_ref and u3 = uniform(key_3)."""
    w = np.ascontiguousarray(w, F)
    u3 = F(u3)
    nb = N // K_BLOCK
    assert w.shape == (N,) and N == nb * K_BLOCK and nb & (nb - 1) == 0 and 2 <= nb <= 256
    w_max, inv_n = w.max(), F(1) / F(N)
    # ---- what k_lg_norm publishes: per tile the tree sum of J_prob with [i*] = 0 and the first w; the sibling sums of i*
    jp = _jprob(w, w_max, inv_n)
    jp[i_ref] = F(0)
    tiles = [_up_sweep(jp[b * K_BLOCK:(b + 1) * K_BLOCK].reshape(64, 4)) for b in range(nb)]
    bsumJ, wfirst = np.zeros(256, F), np.zeros(256, F)
    bsumJ[:nb] = [t["root"] for t in tiles]
    wfirst[:nb] = w[::K_BLOCK]
    b_ref = i_ref // K_BLOCK
    refsib = _sibling_sums(tiles[b_ref], i_ref % K_BLOCK)
    # ---- the tree over the tiles, four tiles per lane
    t = _up_sweep(bsumJ.reshape(64, 4))
    tile_ix = np.arange(256)
    jq = _jprob(wfirst, w_max, inv_n)
    Ji = max(F(1) - t["root"], F(0))
    jf = np.where(tile_ix * K_BLOCK == i_ref, Ji, np.where(tile_ix < nb, jq, F(0))).astype(F).reshape(64, 4)
    tile_ref = _fold(Ji, refsib)
    bsib = _sibling_sums(t, b_ref)
    rootJ = _fold(tile_ref, bsib)
    q = rootJ * (F(1) - u3)
    wk = _Walk(q, rootJ)
    lo = 0
    for c in range(nb.bit_length() - 2, -1, -1):
        mid = lo + (1 << c)
        left = _fold(tile_ref, bsib, c) if lo <= b_ref < mid else _half(t, lo, c)
        lo = lo if wk.left(left, _mid(jf, lo, c)) else mid
    # ---- the tile of J, rebuilt from w with leaf i* = Ji
    lo0 = lo * K_BLOCK
    x = _jprob(w[lo0:lo0 + K_BLOCK], w_max, inv_n)
    if lo0 <= i_ref < lo0 + K_BLOCK:
        x[i_ref - lo0] = Ji
    t = _up_sweep(x.reshape(64, 4))
    lo = 0
    for c in range(7, 1, -1):
        lo = lo if wk.left(_half(t, lo, c), _mid(t["x"], lo, c)) else lo + (1 << c)
    x4 = t["x"][lo >> 2]
    g1 = wk.left(t["s01"][lo >> 2], x4[2])       # the node of four leaves
    tt = wk.P + (x4[0] if g1 else x4[2])
    gl = bool(q <= wk.E)                         # two leaves: the probe is E itself
    E = tt if gl else wk.E
    leaf = lo0 + lo + (0 if g1 else 2) + (0 if gl else 1)
    for v in (w_max, inv_n, Ji, tile_ref, rootJ, q, wk.P, wk.E, tt):
        assert isinstance(v, F), "a step left float32"
    return leaf if q <= E else leaf + 1


def oracle_forward(O, om, key, x0, y0, bs, N, eb=True):
    """The stored forward pass of the sweep gibbs_kernel_lg(om, key, x0, y0, bs, N, eb, False) makes: the oracle's own
    csmc_forward_pass_lg under the keys of gibbs.py:126-148.  Returns (pass, key of the pass)."""
    du = om.du
    k3 = O.split(key, 3)
    path = O.lg_fwd_sampler(om, k3[0], np.concatenate([x0, y0]).astype(F))[::-1]
    us, vs = np.ascontiguousarray(path[:, :du]), np.ascontiguousarray(path[:, du:])
    kf = O.split(k3[1], 4 if eb else 2)[0]
    us0 = np.repeat(us[:1], N, axis=0)
    lw0 = np.full(N, F(-np.log(float(N))), F)
    return O.csmc_forward_pass_lg(om, kf, us, bs, vs, us0, lw0), kf


def oracle_steps(O, om, key, x0, y0, bs, N, eb=True):
    """For every step s of that sweep: dict(w, i_ref, u3, J) -- the normalised weights the resampler of step s sees, its
    reference index, the uniform of its J draw and the oracle's own J.  J is the oracle's choice() over the oracle's J_prob
    (csmc/resamplings.py:79-84 with the oracle's division, sum and key split), and wherever most slots survive it is
    checked against the roll read off the oracle's ancestors (a slot neither killed nor pinned has ancestor m - (j* - J))."""
    fwd, kf = oracle_forward(O, om, key, x0, y0, bs, N, eb)
    keys = O.split(O.split(kf, 2)[1], om.T)
    out = []
    for s in range(om.T):
        w = O.exp(fwd["log_wss"][s])
        i_ref = int(bs[s])
        k3 = O.split(O.split(keys[s], 2)[0], 3)
        jp = O.div(F(1) - O.div(w, np.full(N, w.max(), F)), np.full(N, F(N), F))
        jp[i_ref] = F(0)
        jp[i_ref] = max(F(1) - O.tree_sum(jp), F(0))
        J = int(O.choice(k3[2], jp))
        votes = np.bincount((np.arange(N) - fwd["As"][s]) % N, minlength=N)
        if votes.max() > N // 2:
            assert (int(bs[s + 1]) - int(votes.argmax())) % N == J, f"step {s}: the ancestors' roll disagrees with J"
        out.append(dict(w=w, i_ref=i_ref, u3=F(O.uniform(k3[2])), J=J))
    return out
