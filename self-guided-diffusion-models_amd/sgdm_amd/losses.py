"""The diffusion losses of the drop-in: ``p_losses_hip`` (LatentDiffusion.p_losses, ddpm.py:54-86) and what it is made of.

A step noises the batch, evaluates the model and reduces its output to one loss per sample; ``loss.backward()`` then enters
the UNet's backward program (``train.py``) with the gradient of that reduction.  Which reduction runs is decided once per
step (``_loss_path``):

  * ``"torch"``: the reference's op chain on a target tensor (``simple_loss_torch``).  Its l2 form is ``_MSEFn``, a torch chain
    with a hand-written backward -- NOT the kernel ``sgd_mse_loss``, which only its kernel test calls.  Noising is
    ``sgd_q_sample`` (``sgd_q_sample_v`` with parameterization 'v': x_noisy and the target from one read);
  * ``"weighted_fused"``, hparam ``loss_weighting`` on the device (not in the reference): the per-timestep weighted loss and
    its gradient = ``sgd_loss_fwd`` / ``sgd_loss_bwd`` (``_WeightedLossFn``), the target formed on the fly;
  * ``"lv"``, hparam ``learn_sigma`` (not in the reference): the hybrid loss L_simple + vlb_weight * L_vlb of a 2C-wide model
    output and its gradient = ``sgd_lv_loss_fwd`` / ``sgd_lv_loss_bwd`` (``_LVLossFn``); a torch chain off the device;
  * ``"distill_fused"``, hparam ``distill_guidance`` with a drop-in UNet teacher on the device (not in the reference; Meng et
    al. 2023, stage 1): the loss against the guided output of a frozen teacher and its gradient = ``sgd_distill_loss_fwd`` /
    ``sgd_distill_loss_bwd`` (``_DistillLossFn``), the target formed on the fly from the raw output the teacher's doubled
    evaluation left in its engine.  Any other teacher gives a target tensor and the ``"torch"`` path;
  * ``"progressive_fused"``, hparam ``progressive_steps`` = K with a drop-in UNet teacher on the device (not in the reference;
    Salimans & Ho 2022, Algorithm 2 = stage 2 of Meng et al. 2023): ``t`` is snapped to the K-step trailing grid, the frozen
    teacher is evaluated at (z_t, t), ``sgd_pd_half_step`` forms its DDIM half step z_m and the part of the target known so
    far, the teacher is evaluated again at (z_m, t - T / 2K), and the loss against y* = d0 z_t + d1 y1 + d2 y2 and its gradient
    = ``sgd_pd_loss_fwd`` / ``sgd_pd_loss_bwd`` (``_ProgressiveLossFn``), the target formed on the fly.  With
    ``distill_guidance`` as well each teacher evaluation is the guided one (stages 1 and 2 in one).  Any other teacher: the
    same target as a torch chain (``progressive_target_torch``) and the ``"torch"`` path.

The four kernel pairs share their device core (csrc/loss_common.h).
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .unet import UNetModelBase, _ptr


class _MSEFn(torch.autograd.Function):
    """per-sample mean squared error between noise and eps (ddpm.py:67-75) as a torch chain, forward + hand-written gradient"""

    @staticmethod
    def forward(ctx, eps, target):
        B, Cc, H, W = eps.shape
        per = ((target - eps) ** 2).reshape(B, -1).mean(1)
        ctx.save_for_backward(eps, target)
        return per

    @staticmethod
    def backward(ctx, gper):
        eps, target = ctx.saved_tensors
        B = eps.shape[0]
        chw = eps[0].numel()
        return (-2.0 / chw) * (target - eps) * gper.reshape(B, 1, 1, 1), None


_LOSS_PAR = {"eps": 0, "x0": 1, "v": 2}           # include/sgdm_hip.h: sgd_loss_fwd's par / kind
_LOSS_KIND = {"l2": 0, "l1": 1, "huber": 2}


def _loss_kind(loss_type):
    """the kernels' ``kind`` of the hparam loss_type; the one place an unknown one is refused"""
    if loss_type not in _LOSS_KIND:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    return _LOSS_KIND[loss_type]


def q_sample_dev(s, x0, nz, tt, with_v=False):
    """x_noisy = sa[t] x0 + s1[t] noise on the device (sgd_q_sample) from contiguous fp32 ``x0`` / ``nz`` and int64 ``tt``;
    ``with_v``: (x_noisy, v target) from one read of both (sgd_q_sample_v)"""
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    sa, s1, B, chw = _ptr(s.sqrt_alphas_cumprod), _ptr(s.sqrt_one_minus_alphas_cumprod), x0.shape[0], x0[0].numel()
    x_noisy = torch.empty_like(x0)
    if not with_v:
        L.check(lib.sgd_q_sample(_ptr(x0), _ptr(nz), _ptr(tt), sa, s1, B, chw, _ptr(x_noisy), st), "sgd_q_sample")
        return x_noisy
    v_target = torch.empty_like(x0)
    L.check(lib.sgd_q_sample_v(_ptr(x0), _ptr(nz), _ptr(tt), sa, s1, B, chw, _ptr(x_noisy), _ptr(v_target), st), "sgd_q_sample_v")
    return x_noisy, v_target


def trained_target(s, par, x_start, noise, t):
    """the tensor the model is trained to predict: noise ('eps'), x_start ('x0') or sa[t] * noise - s1[t] * x_start ('v',
    Salimans & Ho 2022); the torch form of what the fused kernels form on the fly (csrc/loss_common.h: loss_target)"""
    if par == "x0":
        return x_start
    if par == "eps":
        return noise
    return (s._ext(s.sqrt_alphas_cumprod, t, x_start.shape) * noise
            - s._ext(s.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * x_start)


def simple_loss_torch(loss_type, target, out, mse_fn=False):
    """the per-sample simple loss as a torch chain (ddpm.py:67-103); ``mse_fn``: l2 through _MSEFn (p_losses_hip's own path:
    one saved pair and a hand-written gradient instead of autograd's chain)"""
    _loss_kind(loss_type)
    if loss_type == "l2":
        return _MSEFn.apply(out, target) if mse_fn else ((target - out) ** 2).reshape(len(target), -1).mean(1)
    if loss_type == "l1":
        return (target - out).abs().reshape(len(target), -1).mean(1)
    return torch.nn.functional.smooth_l1_loss(target, out, reduction="none").reshape(len(target), -1).mean(1)   # huber


class _WeightedLossFn(torch.autograd.Function):
    """(per_w, per_raw) = per-sample loss of the trained target with and without the timestep weight wt[t], one launch
    (sgd_loss_fwd); the gradient for the model output in one more (sgd_loss_bwd).  The target -- noise, x_start or
    sa[t] * noise - s1[t] * x_start -- is formed inside both kernels from the tensors q_sample read: none is written."""

    @staticmethod
    def forward(ctx, out, x0, noise, t, sa, s1, wt, par, kind):
        lib = L.load()
        out = out.contiguous().float()
        B, chw = out.shape[0], out[0].numel()
        per_raw, per_w = (torch.empty(B, dtype=torch.float32, device=out.device) for _ in range(2))
        L.check(lib.sgd_loss_fwd(_ptr(out), _ptr(x0), _ptr(noise), _ptr(t), _ptr(sa), _ptr(s1), _ptr(wt), par, kind, B, chw,
                                 _ptr(per_raw), _ptr(per_w), torch.cuda.current_stream().cuda_stream), "sgd_loss_fwd")
        ctx.save_for_backward(out, x0, noise, t, sa, s1, wt)
        ctx.par, ctx.kind = par, kind
        ctx.mark_non_differentiable(per_raw)
        return per_w, per_raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, _graw):
        out, x0, noise, t, sa, s1, wt = ctx.saved_tensors
        gper = gper.contiguous().float()
        gout = torch.empty_like(out)
        L.check(L.load().sgd_loss_bwd(_ptr(out), _ptr(x0), _ptr(noise), _ptr(t), _ptr(sa), _ptr(s1), _ptr(wt), gper.data_ptr(),
                                      1.0, ctx.par, ctx.kind, out.shape[0], out[0].numel(), _ptr(gout),
                                      torch.cuda.current_stream().cuda_stream), "sgd_loss_bwd")
        return (gout,) + (None,) * 8


# ---- guidance distillation (hparam distill_guidance; Meng et al. 2023, stage 1): the target is the guided output of a frozen
# teacher, in the model's own output space (guidance is linear in it, so every parameterization works unchanged).
class _DistillLossFn(torch.autograd.Function):
    """(per_w, per_raw) = per-sample loss of the student's output against guided(teacher's raw output), with and without the
    timestep weight, one launch (sgd_distill_loss_fwd); the gradient for the student's output in one more
    (sgd_distill_loss_bwd).  ``teach`` is the teacher engine's own output buffer ([2B, hw, C], or the guide pass's [B, hw, C]
    with mode 0) read in place by both kernels: the target is never written, nothing is re-laid.  The backward reads the buffer
    again, so it must run before the teacher's next evaluation at this batch -- the order of every training loop, and the rule
    the student's own backward already imposes (_UNetTrainFn)."""

    @staticmethod
    def forward(ctx, out, teach, mode, w_dev, t, wt, kind):
        lib = L.load()
        out = out.contiguous().float()
        B, Cc, hw = out.shape[0], out.shape[1], out[0, 0].numel()
        per_raw, per_w = (torch.empty(B, dtype=torch.float32, device=out.device) for _ in range(2))
        L.check(lib.sgd_distill_loss_fwd(_ptr(out), _ptr(teach), mode, _ptr(w_dev), _ptr(t), _ptr(wt), kind, B, Cc, hw,
                                         _ptr(per_raw), _ptr(per_w), torch.cuda.current_stream().cuda_stream),
                "sgd_distill_loss_fwd")
        ctx.save_for_backward(out, teach, w_dev, t, wt)
        ctx.mode, ctx.kind = mode, kind
        ctx.mark_non_differentiable(per_raw)
        return per_w, per_raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, _graw):
        out, teach, w_dev, t, wt = ctx.saved_tensors
        gper = gper.contiguous().float()
        gout = torch.empty_like(out)
        L.check(L.load().sgd_distill_loss_bwd(_ptr(out), _ptr(teach), ctx.mode, _ptr(w_dev), _ptr(t), _ptr(wt), ctx.kind,
                                              out.shape[0], out.shape[1], out[0, 0].numel(), gper.data_ptr(), 1.0, _ptr(gout),
                                              torch.cuda.current_stream().cuda_stream), "sgd_distill_loss_bwd")
        return (gout,) + (None,) * 6


# ---- progressive distillation (hparam progressive_steps; Salimans & Ho 2022, Algorithm 2): the target is the output with which
# ONE DDIM step of the student lands where TWO steps of the frozen teacher land, linear in z_t and the teacher's two outputs
# (diffusion.progressive_rows).
class _ProgressiveLossFn(torch.autograd.Function):
    """_DistillLossFn with target = head + d2 * guided(teacher's second raw output): (per_w, per_raw) in one launch
    (sgd_pd_loss_fwd), the gradient for the student's output in one more (sgd_pd_loss_bwd).  ``head`` = d0 z_t + d1 y1 is
    sgd_pd_half_step's; ``teach`` is the teacher engine's own output buffer after its SECOND evaluation, read in place: the
    target is never written.  The backward reads the buffer again (the rule of _DistillLossFn)."""

    @staticmethod
    def forward(ctx, out, head, teach, mode, w_dev, idx, rows, t, wt, kind):
        lib = L.load()
        out = out.contiguous().float()
        B, Cc, hw = out.shape[0], out.shape[1], out[0, 0].numel()
        per_raw, per_w = (torch.empty(B, dtype=torch.float32, device=out.device) for _ in range(2))
        L.check(lib.sgd_pd_loss_fwd(_ptr(out), _ptr(head), _ptr(teach), mode, _ptr(w_dev), idx.data_ptr(), rows.data_ptr(), _ptr(t),
                                    _ptr(wt), kind, B, Cc, hw, _ptr(per_raw), _ptr(per_w),
                                    torch.cuda.current_stream().cuda_stream), "sgd_pd_loss_fwd")
        ctx.save_for_backward(out, head, teach, w_dev, idx, rows, t, wt)
        ctx.mode, ctx.kind = mode, kind
        ctx.mark_non_differentiable(per_raw)
        return per_w, per_raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper, _graw):
        out, head, teach, w_dev, idx, rows, t, wt = ctx.saved_tensors
        gper = gper.contiguous().float()
        gout = torch.empty_like(out)
        L.check(L.load().sgd_pd_loss_bwd(_ptr(out), _ptr(head), _ptr(teach), ctx.mode, _ptr(w_dev), idx.data_ptr(), rows.data_ptr(),
                                         _ptr(t), _ptr(wt), ctx.kind, out.shape[0], out.shape[1], out[0, 0].numel(),
                                         gper.data_ptr(), 1.0, _ptr(gout), torch.cuda.current_stream().cuda_stream),
                "sgd_pd_loss_bwd")
        return (gout,) + (None,) * 9


def progressive_half_step(x, teach, mode, w_dev, idx, rows):
    """(z_mid, head) = (a1 x + b1 g, d0 x + d1 g), g = guided(teach), rows gathered at ``idx``: sgd_pd_half_step, one pass over
    ``x`` (contiguous fp32 NCHW) and the teacher's raw output"""
    B, Cc, hw = x.shape[0], x.shape[1], x[0, 0].numel()
    z_mid, head = torch.empty_like(x), torch.empty_like(x)
    L.check(L.load().sgd_pd_half_step(_ptr(x), _ptr(teach), mode, _ptr(w_dev), idx.data_ptr(), rows.data_ptr(), B, Cc, hw,
                                      _ptr(z_mid), _ptr(head), torch.cuda.current_stream().cuda_stream), "sgd_pd_half_step")
    return z_mid, head


def progressive_target_torch(rows, idx, x, teacher_eval, t, t_mid):
    """the target of progressive distillation as a torch chain, in the dtype of ``x``: ``rows`` [K, >= 5] (a1, b1, d0, d1, d2),
    ``teacher_eval(z, t)`` the teacher's (guided) output.  The CPU branch of p_losses and the restatement the kernels are
    tested against: z_m = a1 x + b1 y1, head = d0 x + d1 y1, y* = head + d2 y2, in the kernels' order"""
    r = rows.to(x.device, x.dtype)[idx]
    a1, b1, d0, d1, d2 = (r[:, k].reshape(-1, *((1,) * (x.dim() - 1))) for k in range(5))
    y1 = teacher_eval(x, t)
    z_mid = a1 * x + b1 * y1
    head = d0 * x + d1 * y1
    y2 = teacher_eval(z_mid, t_mid)
    if y2.shape != x.shape:
        raise ValueError(f"distillation: the teacher's output is {tuple(y2.shape)}, the image {tuple(x.shape)}")
    return head + d2 * y2


def distill_teacher_from(model, ema=None, hip_precision=None):
    """a frozen teacher for guidance distillation from a drop-in UNet: a deep copy of ``model`` (parameters and buffers; no
    engine, workspace or captured step is copied -- the teacher builds its own), with the EMA shadows copied in when ``ema``
    (a LitEma of ``model``) is given, in eval mode with nothing requiring grad, and optionally another arithmetic mode
    (``hip_precision``).  The inference-only modes 'f16' / 'bf16' are allowed: the teacher only ever runs under
    torch.no_grad().  Hand the result to ``LatentDiffusion.set_distill_teacher``."""
    import copy
    if not isinstance(model, UNetModelBase):
        raise TypeError(f"distill_teacher_from copies a drop-in UNet, not {type(model).__name__}")
    if hip_precision is not None and hip_precision not in L.PREC_BY_NAME:
        raise ValueError(f"hip_precision={hip_precision!r}: one of {sorted(L.PREC_BY_NAME)}")
    # what belongs to ``model``'s device state stays behind: the copy starts with empty caches
    memo = {id(model.__dict__[k]): {} for k in ("_engines", "_hip_graph_steps") if k in model.__dict__}
    # (the ``condition`` node of the config is read only and shared: attribute-style dict classes often cannot be deep-copied)
    memo[id(model.condition)] = model.condition
    teacher = copy.deepcopy(model, memo)
    teacher._engines = {}
    teacher.__dict__.pop("_hip_graph_steps", None)
    teacher.__dict__.pop("_tensor_list", None)
    if ema is not None:
        ema.copy_to(teacher)                    # (the copy still has ``model``'s requires_grad flags, which name the shadows)
    teacher.eval().requires_grad_(False)
    if hip_precision is not None:
        teacher.hip_precision = hip_precision
    return teacher


def _distill_setup(diff, student, kwargs, device):
    """the checks of a distillation step, all before anything is launched: (w, phi, teacher UNet or None, teacher callable).
    ``student``: the UNet behind denoise_fn when it is one.  ValueError: no teacher; learned variance on either model;
    out_channels that differ; teacher and student the same object; a teacher that is in train mode or has parameters that
    require grad; a caller's cond_drop_mask (the student is trained on its conditional branch alone); distill_rescale off
    the fused path (the rescale needs both halves of the teacher's doubled evaluation)."""
    # (progressive_steps without distill_guidance: w is None -- the teacher is evaluated once, conditionally, not guided)
    w, phi = diff.distill if diff.distill is not None else (None, 0.0)
    teacher = getattr(diff, "_distill_teacher", None)
    if teacher is None:
        raise ValueError(f"{'distill_guidance' if w is not None else 'progressive_steps'} is set but there is no teacher: call "
                         "set_distill_teacher(teacher) first (sgdm_amd.train.distill_teacher_from copies one from a drop-in UNet)")
    owner = getattr(teacher, "__self__", teacher)
    if owner is student or teacher is diff.denoise_fn or owner is diff.denoise_fn:
        raise ValueError("distillation: teacher and student are the same object; the teacher must be a frozen copy "
                         "(sgdm_amd.train.distill_teacher_from)")
    if getattr(diff.sampler, "learn_sigma", False) or getattr(owner, "learn_sigma", False):
        raise ValueError("distillation of learned-variance models (learn_sigma) is not implemented")
    oc_t, oc_s = getattr(owner, "out_channels", None), getattr(student, "out_channels", None)
    if oc_t is not None and oc_s is not None and oc_t != oc_s:
        raise ValueError(f"distillation: the teacher has {oc_t} output channels, the student {oc_s}")
    if isinstance(owner, torch.nn.Module):
        if owner.training:
            raise ValueError("distillation: the teacher is in train mode; call teacher.eval() (dropout must be off)")
        if any(p.requires_grad for p in owner.parameters()):
            raise ValueError("distillation: the teacher has parameters that require grad; call teacher.requires_grad_(False)")
    if kwargs.get("cond_drop_mask") is not None:
        raise ValueError("distillation trains the student's conditional evaluation alone (cond_drop_prob is forced to 0): "
                         "a cond_drop_mask cannot be honoured")
    unet = owner if isinstance(owner, UNetModelBase) and device.type == "cuda" else None
    if unet is not None and getattr(teacher, "__name__", "forward_with_cond_scale") != "forward_with_cond_scale":
        unet = None                                 # some other bound method of a UNet: called as it is
    if w is None and unet is None:                  # one plain evaluation: the teacher itself, called without a weight
        return w, phi, unet, teacher
    if phi > 0 and unet is None:
        raise ValueError("distill_rescale needs the fused path: a drop-in UNet teacher on the device (the rescale reads both "
                         "halves of its doubled evaluation)")
    fn = teacher if owner is not teacher or not hasattr(teacher, "forward_with_cond_scale") else teacher.forward_with_cond_scale
    return w, phi, unet, fn


def _distill_teacher_eval(diff, unet, w, phi, x_noisy, t, kwargs):
    """the fused path: the teacher's doubled evaluation under no_grad, its raw output left where the engine wrote it.
    Returns (teach buffer, cfg_mode, device float w): ``eng.eps_nhwc`` [2B, hw, C] with the teacher's scale type, or with
    distill_rescale the guide pass's [B, hw, C] and mode 0; with ``w`` None (progressive distillation without
    distill_guidance) ONE conditional evaluation: ``eng.eps_nhwc`` [B, hw, C], mode 0 and no weight."""
    from .diffusion import _StepRunner
    runner = diff.__dict__.get("_distill_runner")
    if runner is None or runner.model is not unet:
        runner = diff.__dict__["_distill_runner"] = _StepRunner(
            unet.forward_with_cond_scale, *((dict(cond_scale=w),) if w is not None else ({}, dict(cfg_distilled=True))))
        runner.w_dev = {}
    dev = x_noisy.device
    if w is None:
        # progressive distillation of an already distilled teacher: ONE conditional evaluation at B, mode 0, no weight (the
        # evaluation a cfg_distilled sampling step runs: _StepRunner.eps)
        with torch.no_grad():
            mask = unet._draw_mask(x_noisy.shape[0], 0.0, dev) if runner.cond_only_mask() else None
            eng = unet._run(x_noisy, t, kwargs.get("cond"), kwargs.get("layout"), mask, x_noisy.shape[0])
        return eng.eps_nhwc, 0, None
    if dev not in runner.w_dev:
        runner.w_dev[dev] = torch.full((1,), w, dtype=torch.float32, device=dev)
    w_dev = runner.w_dev[dev]
    B, Cc, hw = x_noisy.shape[0], x_noisy.shape[1], x_noisy[0, 0].numel()
    with torch.no_grad():
        has_mask, p = runner.drop_mask(B, dev)      # [never | always]: rows [0, B) conditional, [B, 2B) dropped
        mask = unet._draw_mask(2 * B, p, dev) if has_mask else None
        eng = unet._run(x_noisy, t, kwargs.get("cond"), kwargs.get("layout"), mask, 2 * B)
        teach, mode = eng.eps_nhwc, unet._scale_mode()
        if phi > 0:
            g = torch.empty((B, hw, Cc), device=dev)
            L.check(runner.lib.sgd_cfg_guide(_ptr(teach), mode, _ptr(w_dev), phi, B, Cc, hw, _ptr(g),
                                             torch.cuda.current_stream().cuda_stream), "sgd_cfg_guide")
            teach, mode = g, 0
    return teach, mode, w_dev


# ---- learned variance (hparam learn_sigma; Nichol & Dhariwal 2021): L_simple + vlb_weight * L_vlb.  The torch chain below is
# the CPU branch of p_losses and the restatement the device kernels (csrc/lvloss.hip) are tested against; it runs in the
# dtype of its inputs (float64 for gradcheck), except the decoder term, which is always evaluated in double.
_LN2 = math.log(2.0)
_SQRT_2_PI = math.sqrt(2.0 / math.pi)


def lv_coefs(s, t, shape, par):
    """the per-sample schedule scalars of the bound, gathered at ``t`` and shaped to broadcast over ``shape``"""
    names = dict(sa="sqrt_alphas_cumprod", s1="sqrt_one_minus_alphas_cumprod", c1="posterior_mean_coef1",
                 c2="posterior_mean_coef2", mx="lv_max_log", mn="lv_min_log")
    if par == "eps":                    # (infinite on a zero-terminal-SNR table, which 'eps' is refused on)
        names.update(r0="sqrt_recip_alphas_cumprod", r1="sqrt_recipm1_alphas_cumprod")
    return {k: s._ext(getattr(s, v), t, shape) for k, v in names.items()}


def lv_means(par, m, x0, noise, c):
    """(mu_th, mu_q): the posterior means from the model's x0 prediction (not clipped) and from x0 itself"""
    xt = c["sa"] * x0 + c["s1"] * noise
    if par == "eps":
        x0p = c["r0"] * xt - c["r1"] * m
    elif par == "x0":
        x0p = m
    else:
        x0p = c["sa"] * xt - c["s1"] * m
    return c["c1"] * x0p + c["c2"] * xt, c["c1"] * x0 + c["c2"] * xt


def lv_logvar(v, mx, mn):
    frac = (v + 1.0) * 0.5
    return frac * mx + (1.0 - frac) * mn


def lv_kl_bits(mu_th, mu_q, lv, lq):
    """t > 0: KL(q(x_{t-1} | x_t, x0) || p_theta(x_{t-1} | x_t)) per element, in bits"""
    dm = mu_q - mu_th
    e1, e2 = torch.exp(lq - lv), (dm * dm) * torch.exp(-lv)
    return (0.5 * ((((-1.0 + lv) - lq) + e1) + e2)) / _LN2


def lv_decoder_bits(x0, mu_th, lv):
    """t == 0: the discretized-Gaussian decoder NLL of improved-DDPM per element, in bits; evaluated in double (cp - cm
    cancels in fp32 from about four standard deviations out) and returned in the dtype of ``lv``"""
    x, mu, l = x0.double(), mu_th.double(), lv.double()
    inv, d = torch.exp(-0.5 * l), x - mu

    def phi(u):
        return 0.5 * (1.0 + torch.tanh(_SQRT_2_PI * (u + 0.044715 * u * u * u)))

    cp, cm = phi(inv * (d + 1.0 / 255.0)), phi(inv * (d - 1.0 / 255.0))
    p = torch.where(x < -0.999, cp, torch.where(x > 0.999, 1.0 - cm, cp - cm))
    return (-torch.log(p.clamp(min=1e-12)) / _LN2).to(lv.dtype)


def lv_vlb_torch(s, out, x0, noise, t, par):
    """per_vlb [B]: the mean over C*hw of the bound's term at t, bits/dim; the gradient stops at the mean half"""
    Cc = x0.shape[1]
    m, v = out[:, :Cc].detach(), out[:, Cc:]
    c = lv_coefs(s, t, x0.shape, par)
    mu_th, mu_q = lv_means(par, m, x0, noise, c)
    lv = lv_logvar(v, c["mx"], c["mn"])
    kl = lv_kl_bits(mu_th, mu_q, lv, c["mn"])
    dec = lv_decoder_bits(x0.expand_as(mu_th), mu_th, lv)
    first = (t == 0).reshape(-1, *((1,) * (x0.dim() - 1)))
    return torch.where(first, dec, kl).reshape(len(x0), -1).mean(1)


def _lv_tables(s):
    """the host struct of device tables sgd_lv_loss_* take (include/sgdm_hip.h: sgd_lv_tables), from the schedule's buffers"""
    return L.LvTables(sqrt_ac=s.sqrt_alphas_cumprod.data_ptr(), sqrt_1mac=s.sqrt_one_minus_alphas_cumprod.data_ptr(),
                      sqrt_recip_ac=s.sqrt_recip_alphas_cumprod.data_ptr(), sqrt_recipm1_ac=s.sqrt_recipm1_alphas_cumprod.data_ptr(),
                      mean_coef1=s.posterior_mean_coef1.data_ptr(), mean_coef2=s.posterior_mean_coef2.data_ptr(),
                      max_log=s.lv_max_log.data_ptr(), min_log=s.lv_min_log.data_ptr())


class _LVLossFn(torch.autograd.Function):
    """(per_w, per_raw, per_vlb) of a learned-variance model's output [B, 2C, H, W] in one launch (sgd_lv_loss_fwd); the
    gradient for the output -- sgd_loss_bwd's on the mean half, the bound's on the variance half -- in one more
    (sgd_lv_loss_bwd), which is never entered under no_grad."""

    @staticmethod
    def forward(ctx, out, x0, noise, t, sched, wt, par, kind):
        lib = L.load()
        out = out.contiguous().float()
        B, Cc, hw = x0.shape[0], x0.shape[1], x0[0, 0].numel()
        per_raw, per_w, per_vlb = (torch.empty(B, dtype=torch.float32, device=out.device) for _ in range(3))
        tabs = _lv_tables(sched)
        L.check(lib.sgd_lv_loss_fwd(_ptr(out), _ptr(x0), _ptr(noise), _ptr(t), C.byref(tabs), _ptr(wt), par, kind, B, Cc, hw,
                                    _ptr(per_raw), _ptr(per_w), _ptr(per_vlb), torch.cuda.current_stream().cuda_stream),
                "sgd_lv_loss_fwd")
        ctx.save_for_backward(out, x0, noise, t, wt)
        ctx.sched, ctx.par, ctx.kind = sched, par, kind
        ctx.mark_non_differentiable(per_raw)
        return per_w, per_raw, per_vlb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gper_w, _graw, gper_vlb):
        out, x0, noise, t, wt = ctx.saved_tensors
        gper_w, gper_vlb = gper_w.contiguous().float(), gper_vlb.contiguous().float()
        gout = torch.empty_like(out)
        tabs = _lv_tables(ctx.sched)
        L.check(L.load().sgd_lv_loss_bwd(_ptr(out), _ptr(x0), _ptr(noise), _ptr(t), C.byref(tabs), _ptr(wt), gper_w.data_ptr(),
                                         gper_vlb.data_ptr(), ctx.par, ctx.kind, x0.shape[0], x0.shape[1], x0[0, 0].numel(),
                                         _ptr(gout), torch.cuda.current_stream().cuda_stream), "sgd_lv_loss_bwd")
        return (gout,) + (None,) * 7


def lv_loss(s, h, out, x0, noise, t, weights):
    """(per_w, per_raw, per_vlb) of a learned-variance model's output: the fused kernels on the device, the torch chain
    elsewhere"""
    Cc = x0.shape[1]
    if out.dim() != x0.dim() or out.shape[1] != 2 * Cc:
        raise ValueError(f"learn_sigma: the model output has {out.shape[1]} channels, the image {Cc}: a UNet with "
                         f"out_channels == {2 * Cc} is needed")
    kind, par = _loss_kind(h.loss_type), h.parameterization
    if x0.device.type == "cuda":
        return _LVLossFn.apply(out, x0, noise, t, s, weights, _LOSS_PAR[par], kind)
    raw = simple_loss_torch(h.loss_type, trained_target(s, par, x0, noise, t), out[:, :Cc])
    per_w = raw if weights is None else raw * weights[t]
    return per_w, raw.detach(), lv_vlb_torch(s, out, x0, noise, t, par)


@torch.no_grad()
def lv_terms(diff, x_start, t, noise, cond_kwargs):
    """(per_w, per_raw, per_vlb) at ``t`` without gradients: q_sample, one evaluation of ``denoise_fn``, the loss's forward
    (LatentDiffusion.calc_bpd)"""
    s, h = diff.sampler, diff.hparams
    x0, nz, tt = x_start.contiguous().float(), noise.contiguous().float(), t.contiguous().to(torch.int64)
    if x0.device.type == "cuda":
        x_noisy = q_sample_dev(s, x0, nz, tt)
    else:
        x_noisy = s.q_sample(original_sample=x0, t=tt, noise=nz)
    out = diff.denoise_fn(x_noisy, tt, **cond_kwargs)
    out = out[0] if isinstance(out, (tuple, list)) else out
    weights = s.loss_weights if getattr(s, "loss_weighting", None) is not None else None
    return lv_loss(s, h, out, x0, nz, tt, weights)


def _loss_path(lv, distilling, distill_unet, weights, on_dev, progressive=False):
    """which reduction of the model output a step runs (the module docstring), one value decided before the first launch.
    Only "torch" reads a target tensor; the others form theirs inside their kernels ("lv": inside lv_loss, which has a torch
    branch of its own off the device).  A distillation step never takes "weighted_fused": those kernels form the TRAINED
    target, not the teacher's; with a teacher that is not a drop-in UNet on the device it is "torch" on the teacher's tensor.
    ``progressive`` (hparam progressive_steps, with or without distill_guidance): the same rule with the two-step target."""
    if lv:
        return "lv"
    if progressive:                     # (refused with learned variance: diffusion.progressive_option)
        return "progressive_fused" if distill_unet is not None else "torch"
    if distilling:
        return "distill_fused" if distill_unet is not None else "torch"
    return "weighted_fused" if weights is not None and on_dev else "torch"


def per_sample_loss(path, kind, diff, model_output, target, teach, dev, x_start, noise, t, weights):
    """(per_w, raw, vlb): the per-sample loss the gradient flows from, timestep weights applied; the unweighted one when
    weighting is on, else None; the per-sample variational-bound term in bits/dim on the "lv" path, else None.
    ``kind``: _loss_kind(loss_type).  ``dev``: (x0, nz, tt), the contiguous fp32 / int64 forms the kernels read, or None off
    the device."""
    s, h = diff.sampler, diff.hparams
    if path == "lv":
        per_w, raw, vlb = lv_loss(s, h, model_output, *(dev or (x_start, noise, t)), weights)
        return per_w, raw if weights is not None else None, vlb
    if path == "distill_fused":
        if model_output.shape != x_start.shape:
            raise ValueError(f"distillation: the student's output is {tuple(model_output.shape)}, the image "
                             f"{tuple(x_start.shape)}")
        per_w, raw = _DistillLossFn.apply(model_output, *teach, dev[2], weights, kind)
        return per_w, raw if weights is not None else None, None
    if path == "progressive_fused":
        if model_output.shape != x_start.shape:
            raise ValueError(f"distillation: the student's output is {tuple(model_output.shape)}, the image "
                             f"{tuple(x_start.shape)}")
        per_w, raw = _ProgressiveLossFn.apply(model_output, *teach, dev[2], weights, kind)
        return per_w, raw if weights is not None else None, None
    if path == "weighted_fused":
        per_w, raw = _WeightedLossFn.apply(model_output, *dev, s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod, weights,
                                           _LOSS_PAR[h.parameterization], kind)
        return per_w, raw, None
    per = simple_loss_torch(h.loss_type, target, model_output, mse_fn=True)
    if weights is None:
        return per, None, None
    return per * weights[t], per.detach(), None     # the same weights on the torch chain


def refuse_inference_only(model):
    """the single-product modes (hip_precision 'f16' / 'bf16') have no backward: half-precision training needs loss-scale and
    master-weight decisions this library has not made.  Raises before anything is launched."""
    mods = model.modules() if isinstance(model, torch.nn.Module) else ()
    for mod in mods:
        name = getattr(mod, "hip_precision", None)
        if name in L.INFERENCE_ONLY:
            raise ValueError(f"hip_precision='{name}' is inference only (operands rounded once to 16 bits, no backward): "
                             f"train with 'f32', 'f16x3' or 'bf16x3', or run this model under torch.no_grad() / eval()")


def p_losses_hip(diff, x_start, t, noise=None, *args, **kwargs):
    """LatentDiffusion.p_losses (ddpm.py:54-86)"""
    # ---- 1. what is refused, all of it before the first launch
    fn = getattr(diff.denoise_fn, "__self__", diff.denoise_fn)        # the UNet (a bound forward or the module itself)
    if torch.is_grad_enabled() and isinstance(fn, torch.nn.Module) and fn.training and any(p.requires_grad for p in fn.parameters()):
        refuse_inference_only(fn)                                         # a training step
    L.load()
    s, h = diff.sampler, diff.hparams
    noise = torch.randn_like(x_start) if noise is None else noise
    par, on_dev = h.parameterization, x_start.device.type == "cuda"
    if par not in ("eps", "x0", "v"):
        raise NotImplementedError()
    kind = _loss_kind(h.loss_type)
    # hparam loss_weighting (diffusion.loss_weight_table): per-timestep weights on the per-sample loss
    weights = s.loss_weights if getattr(s, "loss_weighting", None) is not None else None
    # hparam distill_guidance: the target is the guided output of the frozen teacher, in the model's own output space; the
    # student is trained on its conditional evaluation alone (cond_drop_prob forced to 0)
    # hparam progressive_steps = K: the target is the output with which one DDIM step of the K-step trailing grid lands where
    # two steps of the frozen teacher land; with distill_guidance each teacher evaluation is the guided one, without it ONE
    # conditional evaluation (the teacher is a distilled student already).  Either way the student trains as in stage 1.
    prog = getattr(diff, "progressive", None)
    dist = getattr(diff, "distill", None)
    dist = dist if dist is not None or prog is None else (None, 0.0)        # (no weight, no rescale: _distill_setup)
    d_unet = None
    if dist is not None:
        d_w, d_phi, d_unet, d_fn = _distill_setup(diff, fn, kwargs, x_start.device)
        if d_unet is not None and d_unet.out_channels != x_start.shape[1]:
            raise ValueError(f"distillation: the teacher has {d_unet.out_channels} output channels, the image {x_start.shape[1]}")
        kwargs = dict(kwargs, cond_drop_prob=0.0)
    # ---- 2. the loss path
    path = _loss_path(getattr(s, "learn_sigma", False), dist is not None, d_unet, weights, on_dev, prog is not None)
    if prog is not None:
        # t snapped to the student's grid, on the device: what q_sample, both models, the weights and the logs see
        from .diffusion import progressive_grid
        T = h.num_timesteps
        p_idx, t = progressive_grid(t.to(torch.int64), prog, T)
        p_idx, t, t_mid = p_idx.contiguous(), t.contiguous(), t - (T // prog) // 2
    # ---- 3. noise; the v target as a tensor only where a torch chain will read it
    want_v = path == "torch" and par == "v" and dist is None
    dev = target = None
    if on_dev:
        dev = x_start.contiguous().float(), noise.contiguous().float(), t.contiguous().to(torch.int64)
        x_noisy = q_sample_dev(s, *dev, with_v=want_v)
        if want_v:
            x_noisy, target = x_noisy
    else:
        x_noisy = s.q_sample(original_sample=x_start, t=t, noise=noise)
    if path == "torch" and dist is None and target is None:
        target = trained_target(s, par, x_start, noise, t)
    # ---- 4. the teacher: its doubled evaluation, the raw output left in its engine, or a callable's guided output
    teach = None
    if path == "distill_fused":
        teach = _distill_teacher_eval(diff, d_unet, d_w, d_phi, x_noisy, dev[2], kwargs)
    elif path == "progressive_fused":
        # teacher at (z_t, t); its half step z_m and the head of the target in one pass; teacher at (z_m, m).  The second
        # evaluation overwrites the first's output in the engine: the head is all the loss needs of it.
        rows = diff.progressive_rows_dev(x_noisy.device)
        teach1, mode, w_dev = _distill_teacher_eval(diff, d_unet, d_w, d_phi, x_noisy, dev[2], kwargs)
        z_mid, head = progressive_half_step(x_noisy, teach1, mode, w_dev, p_idx, rows)
        teach2, mode, w_dev = _distill_teacher_eval(diff, d_unet, d_w, d_phi, z_mid, t_mid, kwargs)
        teach = head, teach2, mode, w_dev, p_idx, rows
    elif dist is not None:
        with torch.no_grad():
            ckw = {k: kwargs[k] for k in ("layout",) if k in kwargs}
            if d_w is not None:
                teacher_eval = lambda z, tt: d_fn(z, tt, d_w, cond=kwargs.get("cond"), **ckw)
            else:                                   # a plain evaluation; a model's (output, loss, dict) triple is accepted
                def teacher_eval(z, tt):
                    y = d_fn(z, tt, cond=kwargs.get("cond"), **ckw)
                    return y[0] if isinstance(y, (tuple, list)) else y
            if prog is None:
                target = teacher_eval(x_noisy, t).detach()
            else:
                from .diffusion import progressive_rows
                rows = progressive_rows(s.alphas_cumprod, prog, par).float()
                target = progressive_target_torch(rows, p_idx, x_noisy, teacher_eval, t, t_mid).detach()
    # ---- 5. the student
    model_output, loss_inside, dict_inside = diff.denoise_fn(x_noisy, t, *args, **kwargs)
    prefix = "train" if diff.training else "val"
    loss_dict = {f"{prefix}/{k}": v for k, v in dict_inside.items()}
    if dist is not None and target is not None and target.shape != model_output.shape:
        raise ValueError(f"distillation: the teacher's output is {tuple(target.shape)}, the student's "
                         f"{tuple(model_output.shape)}")
    # ---- 6. the loss per sample
    loss, raw, vlb = per_sample_loss(path, kind, diff, model_output, target, teach, dev, x_start, noise, t, weights)
    # ---- 7. logging
    if prefix == "train":               # (the UNWEIGHTED per-sample loss: logged per-timestep curves stay comparable)
        loss_dict[f"{prefix}/epoch_stats_y"] = loss.detach() if raw is None else raw
        loss_dict[f"{prefix}/epoch_stats_x"] = t.detach()
    per = loss
    loss = loss.mean()
    loss_dict[f"{prefix}/ddpm_loss"] = loss.detach()
    if raw is not None:
        loss_dict[f"{prefix}/ddpm_loss_raw"] = raw.mean()
    if vlb is not None:                 # ddpm_loss stays the simple term; the bound is logged in bits/dim
        loss_dict[f"{prefix}/vlb"] = vlb.detach().mean()
        loss = (per + s.vlb_weight * vlb).mean()
    loss = loss + loss_inside
    loss_dict[f"{prefix}/loss"] = loss.detach()
    return loss, loss_dict
