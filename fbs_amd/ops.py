"""Device primitives of the sampler hot path on torch (ROCm) tensors, backed by libfbsmi.

``fbs_amd.random``-style PRNG draws follow JAX's threefry semantics (keys are ``uint32[2]`` host
arrays, explicit and stateless like ``jax.random``).  Every function launches HIP kernels on the
current torch stream; none falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

_ws_cache: dict = {}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _require_cuda(t: torch.Tensor, name: str = "tensor") -> None:
    if not t.is_cuda:
        raise RuntimeError(f"fbs_amd: {name} must live on the GPU (got {t.device}); there is no CPU path")


def _ws(n: int, device) -> torch.Tensor:
    """Scratch for the tree kernels, cached per (device, stream) and grown on demand."""
    need = int(_lib.lib().fbsmi_workspace_bytes(int(n)))
    key = (torch.device(device).index, _stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(need, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _f32c(x: torch.Tensor, name="tensor") -> torch.Tensor:
    _require_cuda(x, name)
    if x.dtype != torch.float32:
        x = x.to(torch.float32)
    return x.contiguous()


def _default_device():
    if not torch.cuda.is_available():
        raise RuntimeError("fbs_amd: no GPU visible; the sampler engine has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------
# PRNG (jax.random semantics)
# ------------------------------------------------------------------------------------------------
def PRNGKey(seed: int) -> np.ndarray:
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], dtype=np.uint32)


def _k(key):
    if isinstance(key, torch.Tensor):
        key = key.detach().cpu().numpy()
    k = np.asarray(key, dtype=np.uint32).reshape(2)
    return int(k[0]), int(k[1])


def split(key, num: int = 2) -> np.ndarray:
    """jax.random.split(key, num) -> (num, 2) uint32 host array (pure integer work on the host)."""
    k0, k1 = _k(key)
    out = np.zeros((int(num), 2), dtype=np.uint32)
    _lib.lib().fbsmi_key_split(k0, k1, int(num), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def _numel(shape) -> int:
    if isinstance(shape, int):
        shape = (shape,)
    return int(np.prod(shape, dtype=np.int64)), tuple(shape)


def random_bits(key, shape, device=None) -> torch.Tensor:
    n, shape = _numel(shape)
    out = torch.empty(n, dtype=torch.int32, device=device or _default_device())
    k0, k1 = _k(key)
    _lib.call("fbsmi_random_bits", k0, k1, n, out.data_ptr(), _stream())
    return out.reshape(shape)


def _draw_rows(mode, key, shape, rows, device):
    """Rows [offset, offset+count) of the draw of `shape` (leading axis = rows): identical values to
    slicing the full draw -- what one rank of a sharded ensemble generates."""
    n, shape = _numel(shape)
    offset, count = int(rows[0]), int(rows[1])
    rowlen = n // shape[0] if shape and shape[0] else 0
    out = torch.empty(count * rowlen, dtype=torch.float32, device=device or _default_device())
    k0, k1 = _k(key)
    _lib.call("fbsmi_random_range", mode, k0, k1, n, offset * rowlen, count * rowlen, out.data_ptr(), _stream())
    return out.reshape((count,) + tuple(shape[1:]))


def uniform(key, shape=(), device=None, rows=None) -> torch.Tensor:
    if rows is not None:
        return _draw_rows(1, key, shape, rows, device)
    n, shape = _numel(shape)
    out = torch.empty(n, dtype=torch.float32, device=device or _default_device())
    k0, k1 = _k(key)
    _lib.call("fbsmi_uniform", k0, k1, n, out.data_ptr(), _stream())
    return out.reshape(shape)


def normal(key, shape=(), device=None, rows=None) -> torch.Tensor:
    if rows is not None:
        return _draw_rows(2, key, shape, rows, device)
    n, shape = _numel(shape)
    out = torch.empty(n, dtype=torch.float32, device=device or _default_device())
    k0, k1 = _k(key)
    _lib.call("fbsmi_normal", k0, k1, n, out.data_ptr(), _stream())
    return out.reshape(shape)


def randint(key, shape, minval: int, maxval: int, device=None) -> torch.Tensor:
    n, shape = _numel(shape)
    out = torch.empty(n, dtype=torch.int32, device=device or _default_device())
    k0, k1 = _k(key)
    _lib.call("fbsmi_randint", k0, k1, n, int(minval), int(maxval), out.data_ptr(), _stream())
    return out.reshape(shape)


def categorical(key, weights: torch.Tensor) -> torch.Tensor:
    """jax.random.choice(key, n, (), p=weights) -> int32 scalar tensor (stays on the device)."""
    w = _f32c(weights, "weights").reshape(-1)
    out = torch.empty(1, dtype=torch.int32, device=w.device)
    k0, k1 = _k(key)
    _lib.call("fbsmi_categorical", k0, k1, w.data_ptr(), w.numel(), out.data_ptr(), _ws(w.numel(), w.device).data_ptr(),
              _stream())
    return out.reshape(())


def choice(key, a, shape=(), p=None, axis: int = 0):
    """Subset of jax.random.choice used by the reference: with replacement; ``a`` an int or a tensor
    indexed along axis 0; ``p`` optional weights."""
    n_inputs = int(a) if isinstance(a, int) else a.shape[axis]
    n, shp = _numel(shape)
    if p is None:
        dev = a.device if isinstance(a, torch.Tensor) else _default_device()
        ind = randint(key, shp, 0, n_inputs, device=dev)
    else:
        w = _f32c(p, "p").reshape(-1)
        if n == 1 and shp == ():
            ind = categorical(key, w)
        else:
            c = cumsum(w)
            u = uniform(key, (n,), device=w.device)
            r = c[-1] * (1 - u)
            ind = searchsorted(c, r).reshape(shp)
    if isinstance(a, int):
        return ind
    return torch.index_select(a, axis, ind.reshape(-1).long()).reshape(*shp, *a.shape[1:]) if shp else a[ind.long()]


# ------------------------------------------------------------------------------------------------
# numeric-specification probes
# ------------------------------------------------------------------------------------------------
_MATH_OPS = {"exp": 0, "log": 1, "log1p": 2, "erfinv": 3, "sqrt": 4, "div": 5, "bits_to_normal": 6, "bits_to_normal_kernel": 7, "div_kernel": 8}


def math_map(op: str, x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
    _require_cuda(x, "x")
    x = x.contiguous()
    out = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    yp = _f32c(y).data_ptr() if y is not None else None
    _lib.call("fbsmi_math_map", _MATH_OPS[op], x.data_ptr(), yp, x.numel(), out.data_ptr(), _stream())
    return out.reshape(x.shape)


# ------------------------------------------------------------------------------------------------
# tree reductions / scans
# ------------------------------------------------------------------------------------------------
def cumsum(x: torch.Tensor) -> torch.Tensor:
    """jnp.cumsum of a 1-D float32 tensor in lax.associative_scan order."""
    x = _f32c(x, "x").reshape(-1)
    out = torch.empty_like(x)
    if x.numel():
        _lib.call("fbsmi_cumsum", x.data_ptr(), x.numel(), out.data_ptr(), _ws(x.numel(), x.device).data_ptr(), _stream())
    return out


def tree_sum(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "x").reshape(-1)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.call("fbsmi_sum", x.data_ptr(), x.numel(), out.data_ptr(), _ws(x.numel(), x.device).data_ptr(), _stream())
    return out.reshape(())


def logsumexp(x: torch.Tensor) -> torch.Tensor:
    x = _f32c(x, "x").reshape(-1)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.call("fbsmi_logsumexp", x.data_ptr(), x.numel(), out.data_ptr(), _ws(x.numel(), x.device).data_ptr(), _stream())
    return out.reshape(())


def normalise(log_weights: torch.Tensor, log_space: bool = False, return_lse: bool = False, return_ess: bool = False):
    """fbs/samplers/csmc/csmc.py:273-292.  return_lse / return_ess add the logsumexp (the step's increment of the log
    normalising constant) and the effective sample size 1 / sum w^2 as 0-d device tensors (no host synchronisation)."""
    lw = _f32c(log_weights, "log_weights").reshape(-1)
    out = torch.empty_like(lw)
    lse = torch.empty(1, dtype=torch.float32, device=lw.device)
    if return_ess:
        ess = torch.empty(1, dtype=torch.float32, device=lw.device)
        _lib.call("fbsmi_normalise_ess", lw.data_ptr(), lw.numel(), int(bool(log_space)), out.data_ptr(), lse.data_ptr(),
                  ess.data_ptr(), _ws(lw.numel(), lw.device).data_ptr(), _stream())
        return (out, lse.reshape(()), ess.reshape(())) if return_lse else (out, ess.reshape(()))
    _lib.call("fbsmi_normalise", lw.data_ptr(), lw.numel(), int(bool(log_space)), out.data_ptr(), lse.data_ptr(),
              _ws(lw.numel(), lw.device).data_ptr(), _stream())
    return (out, lse.reshape(())) if return_lse else out


def keys_to_device(keys, device) -> torch.Tensor:
    """(..., 2) uint32 host keys -> an int32 device tensor holding the same bits (what the batched kernels read)."""
    if isinstance(keys, torch.Tensor):
        _require_cuda(keys, "keys")
        return keys.contiguous()
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    return torch.from_numpy(k.view(np.int32)).to(device)


def normalise_batched(log_weights: torch.Tensor, log_space: bool = False, return_lse: bool = False):
    """``normalise`` on every row of log_weights (B, n), n <= 1024, in one launch; row b has the bits of
    ``normalise(log_weights[b])``.  return_lse adds the (B,) logsumexps."""
    lw = _f32c(log_weights, "log_weights")
    if lw.dim() != 2:
        raise ValueError("normalise_batched wants log_weights of shape (B, n)")
    B, n = lw.shape
    out = torch.empty_like(lw)
    lse = torch.empty(B, dtype=torch.float32, device=lw.device) if return_lse else None
    _lib.call("fbsmi_normalise_batched", lw.data_ptr(), B, n, int(bool(log_space)), out.data_ptr(),
              lse.data_ptr() if return_lse else None, _stream())
    return (out, lse) if return_lse else out


def cond_killing_batched(keys, weights: torch.Tensor, i: torch.Tensor, j: torch.Tensor, out=None) -> torch.Tensor:
    """Conditional killing resampling (csmc/resamplings.py:40-88) of B ensembles in one launch: row b of the result
    (B, n) int32 has the bits of ``killing(keys[b], weights[b], i[b], j[b], True)``.  keys (B, 2) uint32 on the host or
    their bits as an int32 device tensor; i, j (B,) integer tensors on the device; n <= 1024.  ``out``: a contiguous
    (B, n) int32 device tensor to write into (a slot of a stored ancestor array) instead of a fresh one."""
    w = _f32c(weights, "weights")
    if w.dim() != 2:
        raise ValueError("cond_killing_batched wants weights of shape (B, n)")
    B, n = w.shape
    kd = keys_to_device(keys, w.device)
    ii, jj = (torch.as_tensor(x, device=w.device).to(torch.int32).contiguous() for x in (i, j))
    if kd.numel() != 2 * B or ii.numel() != B or jj.numel() != B:
        raise ValueError("cond_killing_batched: keys (B, 2), i (B,) and j (B,) must match weights (B, n)")
    if out is None:
        idx = torch.empty((B, n), dtype=torch.int32, device=w.device)
    else:
        idx = out
        if idx.dtype != torch.int32 or tuple(idx.shape) != (B, n) or not idx.is_contiguous() or idx.device != w.device:
            raise ValueError("cond_killing_batched: out must be a contiguous (B, n) int32 tensor on the weights' device")
    _lib.call("fbsmi_cond_killing_batched", kd.data_ptr(), w.data_ptr(), ii.data_ptr(), jj.data_ptr(), B, n,
              idx.data_ptr(), _stream())
    return idx


_RESAMPLE_BATCHED_KINDS = {"stratified": 0, "systematic": 1, "multinomial": 2, "killing": 3}


def resample_batched(weights: torch.Tensor, keys, kind: str = "stratified") -> torch.Tensor:
    """Stratified or systematic resampling (resampling.py:43-58) of B ensembles in one launch: row b of the result (B, n)
    int32 has the bits of ``stratified(weights[b], keys[b])`` / ``systematic(weights[b], keys[b])``.  keys (B, 2) uint32
    on the host or their bits as an int32 device tensor; n <= 1024.  'multinomial' and 'killing' have no batched kernel
    (the library refuses them)."""
    if kind not in _RESAMPLE_BATCHED_KINDS:
        raise ValueError(f"resample_batched: unknown kind {kind!r}")
    w = _f32c(weights, "weights")
    if w.dim() != 2:
        raise ValueError("resample_batched wants weights of shape (B, n)")
    B, n = w.shape
    kd = keys_to_device(keys, w.device)
    if kd.numel() != 2 * B:
        raise ValueError("resample_batched: keys (B, 2) must match weights (B, n)")
    idx = torch.empty((B, n), dtype=torch.int32, device=w.device)
    _lib.call("fbsmi_resample_batched", _RESAMPLE_BATCHED_KINDS[kind], kd.data_ptr(), w.data_ptr(), B, n, idx.data_ptr(),
              _stream())
    return idx


def categorical_batched(keys, weights: torch.Tensor) -> torch.Tensor:
    """``categorical`` on every row of weights (B, n), n <= 1024, in one launch: entry b of the (B,) int32 result has the
    bits of ``categorical(keys[b], weights[b])``.  keys (B, 2) uint32 on the host or their bits as an int32 device tensor."""
    w = _f32c(weights, "weights")
    if w.dim() != 2:
        raise ValueError("categorical_batched wants weights of shape (B, n)")
    B, n = w.shape
    kd = keys_to_device(keys, w.device)
    if kd.numel() != 2 * B:
        raise ValueError("categorical_batched: keys (B, 2) must match weights (B, n)")
    out = torch.empty(B, dtype=torch.int32, device=w.device)
    _lib.call("fbsmi_categorical_batched", kd.data_ptr(), w.data_ptr(), B, n, out.data_ptr(), _stream())
    return out


def force_move_batched(keys, weights: torch.Tensor, k, return_alpha: bool = False):
    """Forced-move selection (gibbs.py:171-214) of B ensembles in one launch: entry b of the (B,) int32 result has the
    bits of ``force_move(keys[b], weights[b], k[b])``'s index.  keys (B, 2) uint32 on the host or their bits as an int32
    device tensor; weights (B, n), n <= 1024; k (B,) integers (a device tensor is not read back).  return_alpha adds the
    (B,) float32 acceptance sums, which are not computed otherwise."""
    w = _f32c(weights, "weights")
    if w.dim() != 2:
        raise ValueError("force_move_batched wants weights of shape (B, n)")
    B, n = w.shape
    kd = keys_to_device(keys, w.device)
    kk = torch.as_tensor(k, device=w.device).to(torch.int32).reshape(-1).contiguous()
    if kd.numel() != 2 * B or kk.numel() != B:
        raise ValueError("force_move_batched: keys (B, 2) and k (B,) must match weights (B, n)")
    out = torch.empty(B, dtype=torch.int32, device=w.device)
    alpha = torch.empty(B, dtype=torch.float32, device=w.device) if return_alpha else None
    _lib.call("fbsmi_force_move_batched", kd.data_ptr(), w.data_ptr(), kk.data_ptr(), B, n, out.data_ptr(),
              alpha.data_ptr() if return_alpha else None, _stream())
    return (out, alpha) if return_alpha else out


def randint_batched(keys, n: int, minval: int, maxval: int, device=None) -> torch.Tensor:
    """Row b of the (B, n) int32 result has the bits of ``randint(keys[b], (n,), minval, maxval)``, in one launch.  keys
    (B, 2) uint32 on the host or their bits as an int32 device tensor."""
    dev = keys.device if isinstance(keys, torch.Tensor) else (device or _default_device())
    kd = keys_to_device(keys, dev)
    B, n = kd.numel() // 2, int(n)
    out = torch.empty((B, n), dtype=torch.int32, device=dev)
    _lib.call("fbsmi_randint_batched", kd.data_ptr(), B, n, int(minval), int(maxval), out.data_ptr(), _stream())
    return out


def backscan_batched(keys, log_w_T: torch.Tensor, As: torch.Tensor, uss: torch.Tensor):
    """``backward_scanning_pass`` (csmc/csmc.py) of B ensembles in one launch.  keys (B, 2) uint32 on the host or their bits
    as an int32 device tensor; log_w_T (B, n), n <= 1024; As (T, B, n) int32 and uss (T + 1, B, n, ...) float32 time-major,
    as the forward pass stores them.  -> (path (B, T + 1, ...), Bs (B, T + 1) int32); ensemble b has the bits of
    ``backward_scanning_pass(keys[b], As[:, b], uss[:, b], log_w_T[b])``."""
    lw = _f32c(log_w_T, "log_w_T")
    u = _f32c(uss, "uss")
    if lw.dim() != 2 or u.dim() < 3:
        raise ValueError("backscan_batched wants log_w_T (B, n) and uss (T + 1, B, n, ...)")
    B, n = lw.shape
    T = int(u.shape[0]) - 1
    if T < 0 or tuple(u.shape[1:3]) != (B, n):
        raise ValueError("backscan_batched: uss must be (T + 1, B, n, ...) with log_w_T's B and n")
    tail = tuple(u.shape[3:])
    du = int(np.prod(tail, dtype=np.int64)) if tail else 1
    A = As.to(torch.int32).contiguous()
    _require_cuda(A, "As")
    if tuple(A.shape) != (T, B, n):
        raise ValueError("backscan_batched: As must be (T, B, n)")
    kd = keys_to_device(keys, lw.device)
    if kd.numel() != 2 * B:
        raise ValueError("backscan_batched: keys (B, 2) must match log_w_T (B, n)")
    Bs = torch.empty((B, T + 1), dtype=torch.int32, device=lw.device)
    path = torch.empty((B, T + 1) + tail, dtype=torch.float32, device=lw.device)
    _lib.call("fbsmi_backscan_batched", kd.data_ptr(), lw.data_ptr(), A.data_ptr() if T else None, u.data_ptr(), B, n, T, du,
              Bs.data_ptr(), path.data_ptr(), _stream())
    return path, Bs


def backsim_pick_batched(keys, lw: torch.Tensor, us: torch.Tensor, log_w=None, out=None, idx=None):
    """One step of backward simulation for B ensembles in one launch (fbsmi_backsim_pick_batched): with g = lw[b], or
    (g - max(g)) + log_w[b] when log_w is given, ensemble b draws i = categorical(keys[b], normalise(g)) and picks the row
    us[b][i].  keys (B, 2) uint32 on the host or their bits as an int32 device tensor; lw, log_w (B, n), n <= 1024; us
    (B, n, ...) float32 whose ensembles are contiguous (n, ...) blocks a fixed stride apart (a time slice of a stored
    (B, T + 1, n, ...) or (T + 1, B, n, ...) array is read in place).  ``out``: a (B, ...) float32 view with contiguous
    rows a fixed stride apart (a slot of a (B, T + 1, ...) trajectory), ``idx``: a (B,) int32 view (a column of a
    (B, T + 1) array); fresh tensors when omitted.  -> (rows (B, ...), indices (B,) int32); ensemble b has the bits of
    ``normalise`` + ``categorical`` + the row gather on its own arrays."""
    lw2 = _f32c(lw, "lw")
    if lw2.dim() != 2:
        raise ValueError("backsim_pick_batched wants lw of shape (B, n)")
    B, n = lw2.shape
    dev = lw2.device
    _require_cuda(us, "us")
    if us.dtype != torch.float32 or us.dim() < 2 or tuple(us.shape[:2]) != (B, n):
        raise ValueError("backsim_pick_batched: us must be float32 (B, n, ...)")
    tail = tuple(us.shape[2:])
    du = int(np.prod(tail, dtype=np.int64)) if tail else 1
    if not us[0].is_contiguous() or (B > 1 and us.stride(0) < 0):
        us = us.contiguous()
    us_stride = int(us.stride(0)) if B > 1 else n * du
    lg = None
    if log_w is not None:
        lg = _f32c(log_w, "log_w")
        if tuple(lg.shape) != (B, n):
            raise ValueError("backsim_pick_batched: log_w must match lw (B, n)")
    kd = keys_to_device(keys, dev)
    if kd.numel() != 2 * B:
        raise ValueError("backsim_pick_batched: keys (B, 2) must match lw (B, n)")
    if out is None:
        out = torch.empty((B,) + tail, dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or tuple(out.shape) != (B,) + tail or out.device != dev or not out[0].is_contiguous() \
            or (B > 1 and out.stride(0) < du):
        raise ValueError("backsim_pick_batched: out must be float32 (B, ...) on lw's device with contiguous rows")
    if idx is None:
        idx = torch.empty(B, dtype=torch.int32, device=dev)
    if idx.dtype != torch.int32 or tuple(idx.shape) != (B,) or idx.device != dev or (B > 1 and idx.stride(0) < 1):
        raise ValueError("backsim_pick_batched: idx must be int32 (B,) on lw's device")
    _lib.call("fbsmi_backsim_pick_batched", kd.data_ptr(), lw2.data_ptr(), lg.data_ptr() if lg is not None else None,
              us.data_ptr(), us_stride, B, n, du, idx.data_ptr(), int(idx.stride(0)) if B > 1 else 1, out.data_ptr(),
              int(out.stride(0)) if B > 1 else du, _stream())
    return out, idx


def searchsorted(a: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    a = _f32c(a, "a").reshape(-1)
    qq = _f32c(q, "q")
    out = torch.empty(qq.numel(), dtype=torch.int32, device=a.device)
    _lib.call("fbsmi_searchsorted", a.data_ptr(), a.numel(), qq.data_ptr(), qq.numel(), out.data_ptr(), _stream())
    return out.reshape(qq.shape)


# ------------------------------------------------------------------------------------------------
# data movement
# ------------------------------------------------------------------------------------------------
def take_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """jnp.take(src, idx, axis=0) for a float32 tensor of any trailing shape."""
    _require_cuda(src, "src")
    if src.dtype != torch.float32:
        return torch.index_select(src, 0, idx.long())
    s = src.contiguous()
    i = idx.to(torch.int32).contiguous()
    d = int(np.prod(s.shape[1:], dtype=np.int64)) if s.dim() > 1 else 1
    out = torch.empty((i.numel(),) + tuple(s.shape[1:]), dtype=torch.float32, device=s.device)
    _lib.call("fbsmi_gather_rows", s.data_ptr(), i.data_ptr(), i.numel(), d, out.data_ptr(), _stream())
    return out


def set_row(dst: torch.Tensor, row: int, value: torch.Tensor) -> torch.Tensor:
    """x.at[row].set(value): functional (returns a new tensor)."""
    out = _f32c(dst, "dst").clone()
    v = _f32c(value.to(out.device) if isinstance(value, torch.Tensor) else torch.as_tensor(value, device=out.device))
    d = int(np.prod(out.shape[1:], dtype=np.int64)) if out.dim() > 1 else 1
    v = v.expand(out.shape[1:]).contiguous() if out.dim() > 1 else v.reshape(1)
    _lib.call("fbsmi_set_row", out.data_ptr(), int(row), v.data_ptr(), d, _stream())
    return out


def backtrace(As: torch.Tensor, B_T: torch.Tensor) -> torch.Tensor:
    """Bs[T] = B_T; Bs[k-1] = As[k-1, Bs[k]] (csmc.py:262-267)."""
    A = As.to(torch.int32).contiguous()
    _require_cuda(A, "As")
    T, n = A.shape
    b = B_T.to(torch.int32).reshape(1).contiguous()
    out = torch.empty(T + 1, dtype=torch.int32, device=A.device)
    _lib.call("fbsmi_backtrace", A.data_ptr(), T, n, b.data_ptr(), out.data_ptr(), _stream())
    return out
