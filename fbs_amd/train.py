"""The trainer round a score network: fbs/nn/utils.py:60-83 (make_optax_kernel) and experiments/imgs/train.py on the device.

The network's forward and backward pass are PyTorch autograd (with grad enabled fbs_amd/unet.py never reaches libfbsmi's
network kernels).  Everything else of a step is HIP: the loss (fbs_amd/sdes/losses.py), the global gradient norm
(fbsmi_sqnorm) and clip_by_global_norm + adam + the EMA in one pass over the flat parameter vector (fbsmi_adam_ema_step).
The clip norm stays on the device; a step never synchronises with the host.
"""
from __future__ import annotations

import contextlib
import math
import os

import numpy as np
import torch

from . import _lib, ops


# ------------------------------------------------------------------------------------------------
# schedules: optax's formulas as plain host functions of the step count (float64)
# ------------------------------------------------------------------------------------------------
def cosine_decay_schedule(init_value: float, decay_steps: int, alpha: float = 0.0, exponent: float = 1.0):
    """optax.cosine_decay_schedule."""
    if not decay_steps > 0:
        raise ValueError("cosine_decay_schedule: decay_steps must be positive")

    def schedule(count):
        c = min(float(count), float(decay_steps))
        cosine = 0.5 * (1.0 + math.cos(math.pi * c / decay_steps))
        return init_value * ((1.0 - alpha) * cosine ** exponent + alpha)

    return schedule


def exponential_decay(init_value: float, transition_steps: int, decay_rate: float, transition_begin: int = 0,
                      staircase: bool = False, end_value=None):
    """optax.exponential_decay."""
    if not transition_steps > 0:
        raise ValueError("exponential_decay: transition_steps must be positive")

    def schedule(count):
        dec = float(count) - transition_begin
        if dec <= 0:
            return float(init_value)
        p = dec / transition_steps
        if staircase:
            p = math.floor(p)
        val = init_value * decay_rate ** p
        if end_value is not None:
            val = max(val, end_value) if decay_rate < 1.0 else min(val, end_value)
        return val

    return schedule


def constant_schedule(value: float):
    """optax.constant_schedule."""
    return lambda count: float(value)


@contextlib.contextmanager
def torch_own_convolutions():
    """The differentiable pass of the network with the library convolutions switched off (torch's own are used), as in
    fbs_amd/twisted.py: a GPU memory access fault was observed in the library convolutions' backward kernels (DESIGN.md
    section 7), so no differentiable section of this package reaches them."""
    lib_convs = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    try:
        yield
    finally:
        torch.backends.cudnn.enabled = lib_convs


# ------------------------------------------------------------------------------------------------
# flat parameters
# ------------------------------------------------------------------------------------------------
class FlatParams:
    """The module's parameters as views into one flat float32 buffer (`flat`), their .grad as views into a second (`grad`),
    in module.parameters() order, every piece starting on a 16-byte boundary (`numel` counts the padding; it stays zero).

    The fused update writes `flat` through a raw pointer, which torch's version counters do not see; `mark_updated()` bumps
    the version of every parameter so that whatever caches derived weights per version (fbs_amd/unet.py's inference paths)
    rebuilds them.  `sync_grads()` checks after a backward that every .grad still aliases `grad` and copies it in if not."""

    def __init__(self, module: torch.nn.Module):
        self.module = module
        self.params = [p for p in module.parameters()]
        if not self.params:
            raise ValueError("FlatParams: the module has no parameters")
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatParams: every parameter must be float32 and on one device")
        self.offsets, o = [], 0
        for p in self.params:
            self.offsets.append(o)
            o += (p.numel() + 3) // 4 * 4
        self.numel = o
        self.flat = torch.zeros(o, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(o, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                self.flat[off:off + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + p.numel()].view(p.shape)
                p.grad = self.grad[off:off + p.numel()].view(p.shape)

    def views_of(self, vec: torch.Tensor):
        """The pieces of another flat vector of this layout (the EMA, an Adam moment), shaped like the parameters."""
        return [vec[off:off + p.numel()].view(p.shape) for p, off in zip(self.params, self.offsets)]

    def zero_grad(self) -> None:
        self.grad.zero_()
        for p, off in zip(self.params, self.offsets):
            if p.grad is None:
                p.grad = self.grad[off:off + p.numel()].view(p.shape)

    def sync_grads(self) -> int:
        """After backward: gradients that no longer alias the flat buffer are copied into it and re-aliased.  Returns how
        many had to be."""
        moved = 0
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                view = self.grad[off:off + p.numel()].view(p.shape)
                if p.grad is None:
                    view.zero_()
                elif p.grad.data_ptr() != view.data_ptr() or not p.grad.is_contiguous():
                    view.copy_(p.grad)
                    moved += 1
                else:
                    continue
                p.grad = view
        return moved

    def mark_updated(self) -> None:
        """Make writes through the raw pointer visible to version-keyed caches: one version increment per parameter
        (torch._C._increment_version on the list of them; checked with torch 2.10), no pass over the data.  Where that
        private entry is missing or did not count, a bit-preserving in-place multiplication by one does it portably."""
        before = self.params[0]._version
        bump = getattr(torch._C, "_increment_version", None)
        if bump is not None:
            bump(self.params)
        if self.params[0]._version == before:
            with torch.no_grad():
                torch._foreach_mul_(self.params, 1.0)

    def load_vector(self, vec: torch.Tensor) -> None:
        """Overwrite the parameters with another flat vector of this layout (the EMA, before sampling from it)."""
        with torch.no_grad():
            self.flat.copy_(vec)
        self.mark_updated()

    def export(self, vec: torch.Tensor = None) -> torch.Tensor:
        """A flat host vector in the checkpoint order: UNet.export_flat_params order (the reference's ravel_pytree order)
        for a module that has flat_param_spec, module.parameters() order otherwise.  vec: another vector of this layout
        (the EMA); default the parameters themselves."""
        pieces = self.params if vec is None else self.views_of(vec)
        spec = getattr(self.module, "flat_param_spec", None)
        if spec is None:
            return torch.cat([q.detach().reshape(-1).float().cpu() for q in pieces])
        from .unet import ravel_flat_params          # the one place that spells the checkpoint layouts
        by_id = {id(p): q for p, q in zip(self.params, pieces)}
        return ravel_flat_params([(by_id[id(p)], kind) for _, p, kind in spec()])


def sqnorm(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """Sum of squares of a flat float32 device vector as a (1,) device tensor (fbsmi_sqnorm, canonical tree)."""
    ops._require_cuda(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("sqnorm: a contiguous float32 tensor is needed")
    n = x.numel()
    out = torch.empty(1, dtype=torch.float32, device=x.device) if out is None else out
    ws = torch.empty(max(int(_lib.lib().fbsmi_sqnorm_workspace_bytes(n)), 4), dtype=torch.uint8, device=x.device)
    _lib.call("fbsmi_sqnorm", x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ops._stream())
    return out


def adam_ema_step(p, g, m, v, ema, lr, b1, b2, eps, count, gnorm2=None, max_norm=1.0, ema_mode=0, decay=0.0) -> None:
    """One fbsmi_adam_ema_step on flat float32 device vectors; count is optax's (the first step has count 0).  lr and the
    bias corrections 1 - b^(count + 1) are formed in float64 and rounded once."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)) + ((("ema", ema),) if ema is not None else ()):
        ops._require_cuda(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError(f"adam_ema_step: {name} must be a contiguous float32 vector as long as p")
    # b1, b2 as the kernel holds them (float32, as optax's weakly typed decays are): the corrections belong to those values
    t_, b1, b2 = int(count) + 1, float(np.float32(b1)), float(np.float32(b2))
    bc1, bc2 = float(np.float32(1.0 - b1 ** t_)), float(np.float32(1.0 - b2 ** t_))
    _lib.call("fbsmi_adam_ema_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
              None if ema is None else ema.data_ptr(), p.numel(), float(np.float32(lr)), b1,
              b2, float(np.float32(eps)), bc1, bc2, None if gnorm2 is None else gnorm2.data_ptr(),
              float(np.float32(max_norm)), int(ema_mode), float(np.float32(decay)), ops._stream())


def make_adam_kernel(module: torch.nn.Module, loss_fn, learning_rate, grad_clip=None, b1: float = 0.9, b2: float = 0.999,
                     eps: float = 1e-8):
    """(step, ema_kernel) -- fbs/nn/utils.py:60-83 with optax.adam(learning_rate) behind an optional
    optax.clip_by_global_norm(grad_clip).

    step(key, x0s, idx=None) -> the loss as a device tensor: loss_fn(flat_params, key, x0s, idx), backward, the clip norm if
    asked, the fused update.  learning_rate: a number or a schedule of optax's count (0 at the first step).
    ema_kernel(count, count_start, count_every, decay) chooses what the NEXT step does with the EMA, as utils.py:71-81:
    count < count_start copies the new parameters, else every count_every-th count blends, else the EMA is left alone.
    Until ema_kernel is called the EMA is left alone.

    step.params is the FlatParams; step.state holds the flat vectors m, v, ema and the count."""
    fp = FlatParams(module)
    schedule = learning_rate if callable(learning_rate) else constant_schedule(learning_rate)
    dev = fp.flat.device
    state = {"m": torch.zeros_like(fp.flat), "v": torch.zeros_like(fp.flat), "ema": fp.flat.clone(), "count": 0,
             "ema_mode": 0, "decay": 0.0, "gnorm2": torch.zeros(1, dtype=torch.float32, device=dev)}

    def ema_kernel(count: int, count_start: int, count_every: int, decay: float) -> int:
        if count < count_start:
            state["ema_mode"] = 1
        else:
            state["ema_mode"] = 2 if count % count_every == 0 else 0
        state["decay"] = float(decay)
        return state["ema_mode"]

    def step(key, x0s, idx=None):
        fp.zero_grad()
        with torch_own_convolutions(), torch.enable_grad():
            loss = loss_fn(fp, key, x0s, idx)
            loss.backward()
        fp.sync_grads()
        gn2 = None
        if grad_clip is not None:
            gn2 = sqnorm(fp.grad, state["gnorm2"])
        adam_ema_step(fp.flat, fp.grad, state["m"], state["v"], state["ema"], schedule(state["count"]), b1, b2, eps,
                      state["count"], gn2, 1.0 if grad_clip is None else grad_clip, state["ema_mode"], state["decay"])
        fp.mark_updated()
        state["count"] += 1
        return loss.detach()

    step.params, step.state = fp, state
    return step, ema_kernel


def save_checkpoint(path: str, fp: FlatParams, ema: torch.Tensor) -> None:
    """np.savez(path, param=, ema_param=) in UNet.export_flat_params order: what examples/imgs_restore.py loads."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, param=fp.export().numpy(), ema_param=fp.export(ema).numpy())
