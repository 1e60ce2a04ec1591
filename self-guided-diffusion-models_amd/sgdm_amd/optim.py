"""Fused optimizer step of the training loop: AdamW + LitEma in one HIP launch.

Replaces ``torch.optim.AdamW(params, lr, weight_decay)`` of ``configure_optimizers``
(reference lightning_module_common.py:20-42) and the per-step ``LitEma.forward`` (dynamic/ema.py:25-44), which
together issue ~1000 small kernels per step.  ``FusedAdamWEma`` is a ``torch.optim.Optimizer`` (param_groups,
state / state_dict in torch.optim.AdamW's format, LR schedulers such as the reference's LambdaLR work unchanged);
pass the LitEma instance to fold the shadow update into the same kernel and stop calling ``ema(model)``.

Global-norm gradient clipping (``max_grad_norm``, what Lightning's ``gradient_clip_val`` does through
``torch.nn.utils.clip_grad_norm_``) is part of the step: one deterministic norm over every gradient (``sgd_grad_norm``, two
launches), the coefficient stays on the device, and the step multiplies each gradient by it as it loads it
(``sgd_adamw_ema_clip_step``) -- the gradients are not rewritten and the host never waits.  ``clip_grad_norm_`` below is the
same norm followed by an in-place scale, for optimizers that are not this one.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .unet import grad_health

CHUNK = 4096
_ROW_BYTES = 48                       # sizeof(sgd_opt_tensor): five pointers and an int64


def chunk_table(numels):
    """prefix sum of ceil(n / CHUNK): block b of the launch serves the tensor t with start[t] <= b < start[t + 1]"""
    start = [0]
    for n in numels:
        start.append(start[-1] + (int(n) + CHUNK - 1) // CHUNK)
    return start


def _check_max_norm(v):
    """None, or a positive float; inf = measure and guard, never scale"""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"max_grad_norm must be a positive number, inf or None, not {v!r}")
    v = float(v)
    if math.isnan(v) or v <= 0.0:
        raise ValueError(f"max_grad_norm must be a positive number, inf or None, not {v!r}")
    return v


# scratch of sgd_grad_norm: one double per chunk, allocated once per device and size (stream-ordered like any torch tensor)
_PARTIALS = {}


def _partials(dev, total):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(total))
    if key not in _PARTIALS:
        _PARTIALS[key] = torch.empty(int(total), dtype=torch.float64, device=dev)
    return _PARTIALS[key]


def _new_record(dev):
    """a zeroed sgd_clip_record (include/sgdm_hip.h) as int32[8]: norm and coef are its first two words, read as fp32"""
    return torch.zeros(8, dtype=torch.int32, device=dev)


def _record_stats(rec):
    host = rec.cpu()                                              # the one synchronising read
    f = host[:2].view(torch.float32)
    return dict(norm=float(f[0]), coef=float(f[1]), skipped=bool(int(host[2])), clipped_steps=int(host[3]),
                nonfinite_steps=int(host[4]))


def _grad_norm(lib, table_ptr, cstart, count, total, max_norm, rec, dev):
    L.check(lib.sgd_grad_norm(table_ptr, cstart.data_ptr(), count, total, _partials(dev, total).data_ptr(),
                              float(max_norm), rec.data_ptr(), torch.cuda.current_stream().cuda_stream), "sgd_grad_norm")


class FusedAdamWEma(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, ema=None, ema_model=None,
                 max_grad_norm=None):
        """ema: a LitEma whose shadows follow ``ema_model``'s parameters (names resolve the shadow buffers)

        max_grad_norm: clip the global L2 norm of ALL param groups' gradients to this value inside the step; ``float('inf')``
        measures the norm and guards against non-finite gradients without ever scaling; None (the default) issues the launches
        the optimizer issued before.  An attribute (set or clear it at any time), not a ``param_groups`` key: ``state_dict()``
        stays in torch.optim.AdamW's format.  ``p.grad`` is left as it is.  When the norm is not finite the step is void on the
        device -- parameters, moments and shadows keep their values -- exactly as under the health gate, and like there
        ``state[p]['step']`` (a host count of calls) still advances: the bias corrections of later steps count the void one."""
        self.max_grad_norm = max_grad_norm                     # validated before anything else is touched
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema = ema
        self._shadow_of = {}
        if ema is not None:
            if ema_model is None:
                raise ValueError("ema_model is required with ema")
            shadow = dict(ema.named_buffers())
            for name, p in ema_model.named_parameters():
                if p.requires_grad:
                    self._shadow_of[id(p)] = shadow[ema.m_name2s_name[name]]
        self._chunks = {}
        self._clip_rec = {}

    @property
    def max_grad_norm(self):
        return getattr(self, "_max_grad_norm", None)

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self._max_grad_norm = _check_max_norm(v)

    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        raise RuntimeError("FusedAdamWEma has no parameters")

    def _record(self, dev):
        """this optimizer's sgd_clip_record on `dev` (its counters run over the optimizer's life; not optimizer state)"""
        recs = self.__dict__.setdefault("_clip_rec", {})
        if dev not in recs:
            recs[dev] = _new_record(dev)
        return recs[dev]

    @property
    def grad_norm(self):
        """0-dim fp32 DEVICE view of the record's norm: the global gradient norm of the last step taken with max_grad_norm
        set, before clipping (0 before the first).  Reading it does not synchronise; it follows the next step."""
        return self._record(self._device())[:1].view(torch.float32)[0]

    def clip_stats(self):
        """host dict of the record: norm, coef, skipped (the last step), clipped_steps, nonfinite_steps (running).  Syncs."""
        return _record_stats(self._record(self._device()))

    def _chunk_start(self, key, rows, dev):
        if key not in self._chunks:
            start = chunk_table([r[5] for r in rows])
            self._chunks[key] = (torch.tensor(start, dtype=torch.int32, device=dev), start[-1])
        return self._chunks[key]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = L.load()
        omd = -1.0
        if self.ema is not None:
            ema = self.ema
            decay = float(ema.decay)
            if int(ema.num_updates) >= 0:
                ema.num_updates += 1
                n = int(ema.num_updates)
                decay = min(decay, (1 + n) / (10 + n))
            omd = 1.0 - decay
        plans = []                                                # (gi, group, dev, rows, step count, touched) per launch
        keep = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"]]
            if not ps:
                continue
            dev = ps[0].device
            if dev.type != "cuda":
                raise RuntimeError("FusedAdamWEma runs on the GPU only (there is no CPU fallback)")
            rows, step_t, touched = [], None, []
            for p in ps:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamWEma expects contiguous fp32 parameters")
                st = self.state[p]
                g = p.grad
                if g is not None:
                    if not st:
                        st["step"] = torch.tensor(0.0)
                        st["exp_avg"] = torch.zeros_like(p)
                        st["exp_avg_sq"] = torch.zeros_like(p)
                    st["step"] += 1
                    if step_t is not None and float(st["step"]) != step_t:
                        raise RuntimeError("FusedAdamWEma: parameters of one group must share their step count")
                    step_t = float(st["step"])
                    g = g if g.is_contiguous() else g.contiguous()
                    keep.append(g)                                # alive until the launch has consumed it; NOT optimizer
                                                                  # state (state_dict stays torch.optim.AdamW's format)
                    touched.append(p)
                sh = self._shadow_of.get(id(p))
                rows.append((p.data_ptr(), g.data_ptr() if g is not None else 0,
                             st["exp_avg"].data_ptr() if g is not None else 0,
                             st["exp_avg_sq"].data_ptr() if g is not None else 0,
                             sh.data_ptr() if sh is not None else 0, p.numel()))
            if step_t is None and omd < 0:
                continue
            plans.append((gi, group, dev, rows, step_t, touched))
        # the clip: ONE table over the rows of every group (the norm is global), one sgd_grad_norm, and every group's step reads
        # its rows of that table and the one record.  Without it: a table and a launch per group, as before.
        clip = self.max_grad_norm is not None and bool(plans)
        tables = []
        if clip:
            dev = plans[0][2]
            if any(pl[2] != dev for pl in plans):
                raise RuntimeError("FusedAdamWEma: max_grad_norm needs every param group on one device")
            every = [r for pl in plans for r in pl[3]]
            shared = torch.tensor(every, dtype=torch.int64).to(dev, non_blocking=True)
            tables.append(shared)
            cstart, total = self._chunk_start(("all", tuple(r[5] for r in every)), every, dev)
            rec = self._record(dev)
            _grad_norm(lib, shared.data_ptr(), cstart, len(every), total, self.max_grad_norm, rec, dev)
        row0 = 0
        for gi, group, dev, rows, step_t, touched in plans:
            cstart, total = self._chunk_start((gi, tuple(r[5] for r in rows)), rows, dev)
            if clip:
                table_ptr = shared.data_ptr() + _ROW_BYTES * row0
                row0 += len(rows)
            else:
                table = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
                tables.append(table)
                table_ptr = table.data_ptr()
            b1, b2 = group["betas"]
            t = step_t if step_t is not None else 1.0
            # gate (ABI 18): the device's gradient-health flag -- the launch writes nothing while it is up, so gradients a
            # balanced-tail time-out poisoned never reach parameters, moments or EMA shadows (train.Backward.run raises it,
            # the engine's next poll_health() raises on the host and clears it)
            args = (C.c_void_p(table_ptr), C.c_void_p(cstart.data_ptr()), len(rows), total,
                    float(group["lr"]), 1.0 - b1, b2, 1.0 - b2, group["eps"], group["weight_decay"],
                    1.0 - b1 ** t, 1.0 - b2 ** t, omd, C.c_void_p(grad_health(dev).data_ptr()))
            stream = torch.cuda.current_stream().cuda_stream
            if clip:
                L.check(lib.sgd_adamw_ema_clip_step(*args, rec.data_ptr(), stream), "sgd_adamw_ema_clip_step")
            else:
                L.check(lib.sgd_adamw_ema_step(*args, stream), "sgd_adamw_ema_step")
            # The kernel writes the parameters through raw pointers, which autograd's version counters do not see.
            # Every derived copy (packs.Stale: the igemm-packed forward and adjoint weights, the FiLM bias concat, ...) follows
            # the parameters' version counters and must observe the update.
            torch._C._increment_version(touched)
        self._table_keep = (tables, keep)
        return loss


# the record of the free function: one per device (its counters run over the process)
_FREE_RECORD = {}


def clip_grad_norm_(parameters_or_optimizer, max_norm):
    """``torch.nn.utils.clip_grad_norm_`` (L2, global) on the HIP kernels: ``sgd_grad_norm`` then ``sgd_grad_scale`` in place.

    For a Lightning module that overrides ``configure_gradient_clipping`` or an optimizer that is not FusedAdamWEma (which
    clips inside its step: ``max_grad_norm``).  Takes an optimizer (every param group's parameters) or an iterable of
    parameters; gradients that are None are skipped, gradients that are not contiguous fp32 GPU tensors are refused.  Returns
    the total norm before clipping as a 0-dim device tensor; nothing synchronises.  ``max_norm`` of 0 or inf only measures.
    Where torch would multiply a non-finite norm into every gradient, the gradients are left as they are: the returned norm says
    so."""
    if isinstance(parameters_or_optimizer, torch.optim.Optimizer):
        params = [p for group in parameters_or_optimizer.param_groups for p in group["params"]]
    elif isinstance(parameters_or_optimizer, torch.Tensor):
        params = [parameters_or_optimizer]
    else:
        params = list(parameters_or_optimizer)
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)) or math.isnan(float(max_norm)):
        raise ValueError(f"max_norm must be a number, not {max_norm!r}")
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=params[0].device if params else "cpu")
    dev = grads[0].device
    for g in grads:
        if g.device != dev or dev.type != "cuda" or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("clip_grad_norm_ expects contiguous fp32 gradients on one GPU (there is no CPU fallback)")
    lib = L.load()
    rows = [(0, g.data_ptr(), 0, 0, 0, g.numel()) for g in grads]
    start = chunk_table([r[5] for r in rows])
    table = torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
    cstart = torch.tensor(start, dtype=torch.int32).to(dev, non_blocking=True)
    if dev not in _FREE_RECORD:
        _FREE_RECORD[dev] = _new_record(dev)
    rec = _FREE_RECORD[dev]
    _grad_norm(lib, table.data_ptr(), cstart, len(rows), start[-1], max_norm, rec, dev)
    L.check(lib.sgd_grad_scale(table.data_ptr(), cstart.data_ptr(), len(rows), start[-1], rec.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "sgd_grad_scale")
    torch._C._increment_version(grads)                           # written through raw pointers (when coef < 1)
    return rec[:1].view(torch.float32)[0].clone()                # the caller's own copy: the record follows the next call
