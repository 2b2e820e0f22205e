"""The denoising score-matching loss of fbs/sdes/linear.py:230-360 (make_linear_sde_law_loss) on the device.

The key schedule, the random times and the (F, sqrt(Q)) tables are host work (integer ciphers, a sort of a few floats,
float64 closed forms rounded once); they reach the device in ONE asynchronous copy and nothing is read back.  The noising
of the batch and the loss with its derivative are HIP kernels (fbs_amd/csrc/fbsmi_train.hip, specified in include/fbsmi.h)
that draw their noise from the Threefry stream of the row's key; only the network between them is PyTorch, and the loss
sits on its autograd tape through a torch.autograd.Function whose backward is the derivative the forward kernel wrote.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from .linear import LinearSDE, discretise_linear_sde_np

_EPS = 1e-5                      # linear.py:264
_ws_cache: dict = {}


def uniform_host(key, n: int) -> np.ndarray:
    """jax.random.uniform(key, (n,)) as a float32 host array (fbsmi_uniform_host: fbsmi_uniform bit for bit)."""
    k0, k1 = ops._k(key)
    out = np.zeros(int(n), np.float32)
    _lib.call("fbsmi_uniform_host", k0, k1, int(n), out.ctypes.data)
    return out


def uniform_minmax_host(key, n: int, minval: float, maxval: float) -> np.ndarray:
    """jax.random.uniform(key, (n,), minval=, maxval=) in float32 as jax forms it: u * (max - min) + min, then max(min, .)."""
    lo, hi = np.float32(minval), np.float32(maxval)
    return np.maximum(lo, uniform_host(key, n) * np.float32(hi - lo) + lo).astype(np.float32)


def training_times(key_ts, n: int, t0: float, T: float, random_times: bool, save_mem: bool) -> np.ndarray:
    """The float32 times of one loss evaluation.  save_mem (linear.py:324-329): n times, one per row.  Otherwise
    (linear.py:274-279): n + 1 times t_0 .. t_n of the paths, n = nsteps.  The fixed grids are formed in float64 and
    rounded once."""
    if save_mem:
        if random_times:
            return np.concatenate([np.sort(uniform_minmax_host(key_ts, n - 1, t0 + _EPS, T)), np.array([T], np.float32)])
        dt = (T - t0) / n
        return np.linspace(t0 + dt, T, n).astype(np.float32)
    if random_times:
        return np.concatenate([np.array([t0], np.float32), np.sort(uniform_minmax_host(key_ts, n - 1, t0 + _EPS, T)),
                               np.array([T], np.float32)])
    return np.linspace(t0, T, n + 1).astype(np.float32)


def dsm_tables(sde: LinearSDE, t, s, count: int):
    """(F, sq, gc) float32 for rows at float32 times t given time(s) s: F and Q in float64 through
    discretise_linear_sde_np, sq = sqrt(Q), each rounded once; gc = 2 sq / count from the rounded sq, rounded once."""
    F, Q = discretise_linear_sde_np(sde, np.asarray(t, np.float64), np.asarray(s, np.float64))
    F32 = np.asarray(F, np.float64).astype(np.float32)
    sq32 = np.sqrt(np.asarray(Q, np.float64)).astype(np.float32)
    gc32 = (2.0 * sq32.astype(np.float64) / float(count)).astype(np.float32)
    return F32, sq32, gc32


def upload(dev, *arrays):
    """Host arrays of 4-byte elements -> device tensors of the same dtypes, in one asynchronous copy."""
    flat = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.int32) for a in arrays])
    host = torch.from_numpy(flat)
    if torch.device(dev).type == "cuda":
        host = host.pin_memory()
    d = host.to(dev, non_blocking=True)
    out, o = [], 0
    for a in arrays:
        piece = d[o:o + a.size]
        o += a.size
        if a.dtype == np.float32:
            piece = piece.view(torch.float32)
        out.append(piece.reshape(a.shape))
    return out


def _ws(nbytes: int, device) -> torch.Tensor:
    key = (torch.device(device).index, ops._stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _ptr(t):
    return None if t is None else t.data_ptr()


def dsm_noise_batched(data: torch.Tensor, idx, keys_d: torch.Tensor, F: torch.Tensor, sq: torch.Tensor,
                      out_dtype=torch.float32) -> torch.Tensor:
    """xt (B, D) = F[b] data[idx[b]] + sq[b] normal(keys[b], (D,)) (fbsmi_dsm_noise_batched).  data (N, D) float32 on the
    device; idx an int32 device tensor of B rows of data, or None for rows 0 .. B - 1 with B = len(keys)."""
    ops._require_cuda(data, "data")
    if data.dtype != torch.float32 or not data.is_contiguous() or data.dim() != 2:
        raise ValueError("dsm_noise_batched: data must be a contiguous (N, D) float32 tensor")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dsm_noise_batched: out_dtype must be float32 or bfloat16")
    B, D = int(keys_d.shape[0]), int(data.shape[1])
    if idx is None and B > data.shape[0]:
        raise ValueError("dsm_noise_batched: more keys than data rows")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() != B or not idx.is_contiguous()):
        raise ValueError("dsm_noise_batched: idx must be a contiguous int32 tensor with one entry per key")
    xt = torch.empty((B, D), dtype=out_dtype, device=data.device)
    _lib.call("fbsmi_dsm_noise_batched", data.data_ptr(), _ptr(idx), keys_d.data_ptr(), F.data_ptr(), sq.data_ptr(), B, D,
              0 if out_dtype == torch.float32 else 1, xt.data_ptr(), ops._stream())
    return xt


def dsm_loss_batched(net: torch.Tensor, mode: int, keys_d, xt, data, idx, F, sq: torch.Tensor, gc: torch.Tensor,
                     want_rows: bool = False):
    """(loss (1,), dnet like net, row_sums (B,) or None) of fbsmi_dsm_loss_batched; net (B, D) float32 or bfloat16."""
    ops._require_cuda(net, "net")
    if net.dim() != 2 or not net.is_contiguous() or net.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dsm_loss_batched: net must be a contiguous (B, D) float32 or bfloat16 tensor")
    B, D = int(net.shape[0]), int(net.shape[1])
    dev = net.device
    dnet = torch.empty_like(net)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev) if want_rows else None
    ws = _ws(int(_lib.lib().fbsmi_dsm_loss_workspace_bytes(B, D)), dev)
    inv = float(np.float32(1.0 / (float(B) * float(D))))
    _lib.call("fbsmi_dsm_loss_batched", net.data_ptr(), 0 if net.dtype == torch.float32 else 1, int(mode), _ptr(keys_d),
              _ptr(xt), _ptr(data), _ptr(idx), _ptr(F), sq.data_ptr(), gc.data_ptr(), inv, B, D, dnet.data_ptr(), _ptr(rows),
              loss.data_ptr(), ws.data_ptr(), ops._stream())
    return loss, dnet, rows


class _DSMLoss(torch.autograd.Function):
    """forward: the loss kernel, which also writes d loss / d net; backward: that derivative times the incoming gradient."""

    @staticmethod
    def forward(ctx, net, launch):
        loss, dnet = launch(net)
        ctx.save_for_backward(dnet)
        ctx.net_shape = net.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        (dnet,) = ctx.saved_tensors
        return (dnet * grad_output.to(dnet.dtype)).reshape(ctx.net_shape), None


def make_linear_sde_law_loss(sde: LinearSDE, nn_fn, t0=0., T=2., nsteps: int = 100, random_times: bool = True,
                             loss_type: str = 'score', save_mem: bool = False):
    """fbs/sdes/linear.py:230-360.  Returns loss_fn(param, key, x0s, idx=None, debug=None) -> a 0-d device tensor on the
    autograd tape of nn_fn(x, t, param); x of shape (rows, *x0s.shape[1:]), t a float32 device tensor (rows,).

    x0s: the (N, ...) float32 data on the device.  idx: an int32 device tensor (or host array) choosing the rows of the
    batch, which are then gathered inside the kernels; None takes all of x0s as the batch, as the reference does.

    save_mem=True: one time per row; the noise kernel, the network on n rows, the loss kernel redrawing the noise (mode 0).
    save_mem=False: n paths of nsteps points (fbsmi_linear_path_batched, identity layout), the network on nsteps * n rows
    ordered (step, sample), the loss kernel on the stored points (mode 1).  The network input is float32 in both.

    debug: a dict that receives the evaluation's xt, times, tables and per-row sums (which are only computed then)."""
    if loss_type in ('ipf', 'ipf-score'):
        raise NotImplementedError(f"Loss {loss_type} is not implemented: fbs_amd trains the 'score' loss only.")
    if loss_type != 'score':
        raise NotImplementedError(f'Loss {loss_type} not implemented.')
    t0, T, nsteps = float(t0), float(T), int(nsteps)

    def batch_of(x0s, idx):
        ops._require_cuda(x0s, "x0s")
        if x0s.dtype != torch.float32 or not x0s.is_contiguous():
            raise ValueError("loss_fn: x0s must be a contiguous float32 device tensor")
        data = x0s.reshape(x0s.shape[0], -1)
        n = int(x0s.shape[0]) if idx is None else int(np.prod(idx.shape))
        return data, n, tuple(x0s.shape[1:])

    def loss_fn_save_mem(param, key, x0s, idx=None, debug=None):
        data, n, state_shape = batch_of(x0s, idx)
        D = int(data.shape[1])
        key_ts, key_fwd = ops.split(key, 2)
        ts = training_times(key_ts, n, t0, T, random_times, True)
        keys = ops.split(key_fwd, n)
        F, sq, gc = dsm_tables(sde, ts, t0, n * D)
        host = [keys.view(np.int32), F, sq, gc, ts]
        if idx is not None and not isinstance(idx, torch.Tensor):
            host.append(np.ascontiguousarray(idx, np.int32).reshape(-1))
        up = upload(data.device, *host)
        keys_d, F_d, sq_d, gc_d, ts_d = up[:5]
        idx_d = None if idx is None else (idx.reshape(-1).contiguous() if isinstance(idx, torch.Tensor) else up[5])
        xt = dsm_noise_batched(data, idx_d, keys_d, F_d, sq_d, torch.float32)
        net = nn_fn(xt.reshape((n,) + state_shape), ts_d, param)
        rows = {}

        def launch(net_):
            loss, dnet, rows["S"] = dsm_loss_batched(net_.detach().reshape(n, D).contiguous(), 0, keys_d, None, None, None,
                                                     None, sq_d, gc_d, want_rows=debug is not None)
            return loss, dnet.reshape(net_.shape)

        loss = _DSMLoss.apply(net, launch)
        if debug is not None:
            debug.update(xt=xt, ts=ts_d, F=F_d, sq=sq_d, gc=gc_d, keys=keys, idx=idx_d, row_sums=rows.get("S"), net=net)
        return loss

    def loss_fn_paths(param, key, x0s, idx=None, debug=None):
        data, n, state_shape = batch_of(x0s, idx)
        D = int(data.shape[1])
        key_ts, key_fwd = ops.split(key, 2)
        ts = training_times(key_ts, nsteps, t0, T, random_times, False)          # (nsteps + 1,)
        keys = ops.split(key_fwd, n)
        Fk, Sk, _ = dsm_tables(sde, ts[1:], ts[:-1], 1)                            # the steps of the paths
        rows_n = nsteps * n
        F, sq, gc = dsm_tables(sde, ts[1:], ts[0], rows_n * D)                     # (t_k, t_0) of the loss
        rep = lambda a: np.repeat(a, n)                                            # row (k - 1) * n + b
        host = [keys.view(np.int32), Fk, Sk, rep(F), rep(sq), rep(gc), rep(ts[1:]),
                np.tile(np.arange(n, dtype=np.int32), nsteps)]
        if idx is not None and not isinstance(idx, torch.Tensor):
            host.append(np.ascontiguousarray(idx, np.int32).reshape(-1))
        up = upload(data.device, *host)
        keys_d, Fk_d, Sk_d, F_d, sq_d, gc_d, ts_d, rowidx_d = up[:8]
        if idx is None:
            x0 = data[:n]
        else:
            x0 = ops.take_rows(data, idx.reshape(-1).contiguous() if isinstance(idx, torch.Tensor) else up[8])
        buf = torch.empty((nsteps + 1, n, D), dtype=torch.float32, device=data.device)
        _lib.call("fbsmi_linear_path_batched", None, D, Fk_d.data_ptr(), Sk_d.data_ptr(), x0.data_ptr(), None,
                  keys_d.data_ptr(), n, nsteps, 0, buf.data_ptr(), n * D, D, None, 0, 0, ops._stream())
        xt = buf[1:].reshape(rows_n, D)                                            # a view: slots 1 .. nsteps are contiguous
        net = nn_fn(xt.reshape((rows_n,) + state_shape), ts_d, param)
        rows = {}

        def launch(net_):
            loss, dnet, rows["S"] = dsm_loss_batched(net_.detach().reshape(rows_n, D).contiguous(), 1, None, xt, x0,
                                                     rowidx_d, F_d, sq_d, gc_d, want_rows=debug is not None)
            return loss, dnet.reshape(net_.shape)

        loss = _DSMLoss.apply(net, launch)
        if debug is not None:
            debug.update(xt=xt, ts=ts_d, F=F_d, sq=sq_d, gc=gc_d, keys=keys, x0=x0, rowidx=rowidx_d, row_sums=rows.get("S"),
                         net=net)
        return loss

    return loss_fn_save_mem if save_mem else loss_fn_paths
