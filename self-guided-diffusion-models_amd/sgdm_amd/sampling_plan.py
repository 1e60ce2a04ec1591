"""What a sampling trajectory was asked to do, resolved once: the option functions of the sampling kwargs and the frozen
record ``SamplingPlan`` that ``resolve_plan`` builds from them before anything is loaded or launched.  The step objects of
``diffusion.py`` (_StepRunner, the _Update classes, _GraphedStep, _EagerStep) read the plan and never the raw kwargs.  Pure
host code: no device, no library load.  None of this has a counterpart in the reference."""
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

# the defaults of the sampling kwargs this module reads, each stated once (``clip_denoised`` has none: a sampler that clips
# needs it; None: absent)
DEFAULTS = dict(parameterization="eps", v_form="eps", cfg_rescale=0, cfg_interval=None, cfg_distilled=False, pag_scale=0,
                pag_layers=None, pag_drop_cond=None, sag_scale=0, sag_layer=None, sag_threshold=None, sag_blur_sigma=None,
                lv_native=False, native_steps=None, dtp=1, noise_dropout=0, hip_graph=True)


def _opt(sk, key):
    return (sk or {}).get(key, DEFAULTS[key])


def cfg_options(sk, fused=True):
    """(cfg_rescale, cfg_interval) of the sampling kwargs: phi in [0, 1] (0: off) and ``(t_lo, t_hi)`` in training timesteps,
    inclusive (None: guidance on every evaluation).  ValueError for a value out of range and, with an option set, for a step
    that is not the fused-CFG one (``fused``: SamplingPlan.fused) -- the guide pass works on the two halves of the doubled
    evaluation.  The sampling kwarg ``cfg_distilled`` (a guidance-distilled student: every evaluation the conditional one at
    B) is refused with either option -- there is no second half to guide or rescale with --, with the learned-variance
    'native' update and on a step that is not the drop-in UNet's.  Pure host code: no device, no library."""
    sk = sk or {}
    if cfg_distilled_option(sk):
        if _opt(sk, "cfg_interval") is not None or _opt(sk, "cfg_rescale") != 0:
            raise ValueError("cfg_distilled with cfg_interval / cfg_rescale: a distilled student has one (conditional) "
                             "evaluation per step, there is no guidance to schedule or rescale")
        if _opt(sk, "lv_native"):
            raise ValueError("cfg_distilled with the learned-variance 'native' update: distillation of learned-variance "
                             "models is not implemented")
        if not fused:
            raise ValueError("cfg_distilled needs the drop-in UNet's forward_with_cond_scale as denoise_sample_fn (and no p0): "
                             "a generic denoise_sample_fn guides inside the call")
        return 0.0, None
    phi, iv = _opt(sk, "cfg_rescale"), _opt(sk, "cfg_interval")
    if isinstance(phi, bool) or not isinstance(phi, (int, float)) or not 0.0 <= phi <= 1.0:       # (NaN fails the comparison)
        raise ValueError(f"cfg_rescale={phi!r}: a number in [0, 1]")
    if iv is not None:
        ok = isinstance(iv, (tuple, list)) and len(iv) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in iv)
        if not ok or iv[0] > iv[1]:
            raise ValueError(f"cfg_interval={iv!r}: (t_lo, t_hi), two ints in training timesteps with t_lo <= t_hi")
        iv = (int(iv[0]), int(iv[1]))
    if (phi > 0 or iv is not None) and not fused:
        raise ValueError("cfg_rescale / cfg_interval need the fused-CFG step: the drop-in UNet's forward_with_cond_scale, a "
                         "numeric cond_scale that is not its single-evaluation 0 / 1 shortcut, and no p0")
    return float(phi), iv


def cfg_distilled_option(sk):
    """the sampling kwarg ``cfg_distilled`` (default False), a bool.  Pure host code."""
    on = _opt(sk, "cfg_distilled")
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"cfg_distilled={on!r} (True or False)")
    return bool(on)


def pag_scale_option(sk):
    """the sampling kwarg ``pag_scale`` (perturbed-attention guidance, Ahn et al. 2024): a finite number >= 0; 0, the default,
    is off.  ValueError for anything else (a bool included).  Pure host code."""
    s = _opt(sk, "pag_scale")
    if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)) or not 0.0 <= s < float("inf"):
        raise ValueError(f"pag_scale={s!r}: a finite number >= 0 (0: off)")               # (NaN fails the comparison)
    return float(s)


def pag_options(sk, fused=True, model=None):
    """None (off), or ``(s, layers, drop_cond)`` of the sampling kwargs ``pag_scale`` / ``pag_layers`` / ``pag_drop_cond``:
    perturbed-attention guidance, eps_c + s (eps_c - eps_p) with eps_p the SAME network whose self-attention map is the
    identity in ``layers`` -- the cfg form of the step kernels with u := eps_p and w := s, whatever the model's scale_type;
    ``cond_scale`` is not read.  ``layers``: a sorted tuple of attention-layer prefixes of ``model`` -- from 'mid' (default, the
    middle block's attention), 'all', or a list of prefixes.  ``drop_cond`` (default False): the perturbed half also drops the
    condition, drop probabilities (0, 1) as for CFG instead of (0, 0).  ValueError, before anything is loaded or launched, for
    a value out of range, an unknown prefix or a selection of nothing, ``pag_layers`` / ``pag_drop_cond`` without
    ``pag_scale > 0``, ``cfg_distilled`` (one evaluation per step: no second half), a step that is not the drop-in UNet's fused
    one (``fused``: SamplingPlan.fused -- a generic denoise_sample_fn, p0, a tensor cond_scale) and a model whose
    attention is not the self-attention block (unetca_fast, use_spatial_transformer).  Pure host code: no device, no library."""
    sk = sk or {}
    s = pag_scale_option(sk)
    layers, drop = _opt(sk, "pag_layers"), _opt(sk, "pag_drop_cond")
    if s == 0:
        if layers is not None or drop is not None:
            raise ValueError("pag_layers / pag_drop_cond without pag_scale > 0")
        return None
    if cfg_distilled_option(sk):
        raise ValueError("pag_scale with cfg_distilled: a distilled student has one (conditional) evaluation per step, there "
                         "is no perturbed half to guide with")
    if not fused or model is None:
        raise ValueError("pag_scale needs the fused step: the drop-in UNet's forward_with_cond_scale as denoise_sample_fn, no "
                         "p0 and no tensor cond_scale")
    if drop is not None and not isinstance(drop, (bool, np.bool_)):
        raise ValueError(f"pag_drop_cond={drop!r} (True or False)")
    known = model.attention_prefixes()
    if layers is None or (isinstance(layers, str) and layers == "mid"):
        want = [p for p in known if p.startswith("middle_block.")]
    elif isinstance(layers, str) and layers == "all":
        want = known
    elif isinstance(layers, (list, tuple)) and all(isinstance(p, str) for p in layers):
        want = list(layers)
    else:
        raise ValueError(f"pag_layers={layers!r}: 'mid', 'all' or a list of attention-layer prefixes ({known})")
    # the engine's own check of its ``pag`` argument (2: any even UNet batch): the model kind, unknown prefixes, an empty set
    return s, model._pag_set(tuple(sorted(set(want))), 2), bool(drop)


SAG_DEFAULTS = dict(sag_layer="middle_block.1", sag_threshold=1.0, sag_blur_sigma=1.0)
SAG_TAPS = 9                                        # the blur's kernel size, fixed (csrc/sag.hip)


def _real(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def sag_scale_option(sk):
    """the sampling kwarg ``sag_scale`` (self-attention guidance, Hong et al. 2023): a finite number >= 0; 0, the default,
    is off.  ValueError for anything else (a bool included).  Pure host code."""
    s = _opt(sk, "sag_scale")
    if not _real(s) or not 0.0 <= s < float("inf"):                                        # (NaN fails the comparison)
        raise ValueError(f"sag_scale={s!r}: a finite number >= 0 (0: off)")
    return float(s)


def sag_options(sk, fused=True, model=None, shape=None):
    """None (off), or ``(s, layer, psi, sigma)`` of the sampling kwargs ``sag_scale`` / ``sag_layer`` / ``sag_threshold`` /
    ``sag_blur_sigma``: self-attention guidance, o + s (o - o~) with o the conditional evaluation at B and o~ the SAME network
    on the image whose x0 prediction is blurred (9 taps, std ``sigma``, default 1.0) where the attention mass of ``layer``
    (an attention-layer prefix of ``model``; default the middle block's, 'middle_block.1') exceeds ``psi`` (default 1.0), re-noised
    -- the cfg form of the step kernels over the pair [o ; o~] with w := s, whatever the model's scale_type; ``cond_scale`` is
    not read.  ValueError, before anything is loaded or launched, for a value out of range, an unknown ``sag_layer``, the three
    other kwargs without ``sag_scale > 0``, ``pag_scale`` or ``cfg_distilled`` next to it, the learned-variance 'native' update, a
    step that is not the drop-in UNet's fused one (``fused``: SamplingPlan.fused -- a generic denoise_sample_fn, p0, a tensor
    cond_scale), a model whose attention is not the self-attention block (unetca_fast, use_spatial_transformer) and an image
    (``shape``, when the caller knows it) with a side below 5: the reflection pad of the blur must be smaller than the side.
    Pure host code: no device, no library."""
    sk = sk or {}
    s = sag_scale_option(sk)
    given = {k: _opt(sk, k) for k in SAG_DEFAULTS}
    if s == 0:
        if any(v is not None for v in given.values()):
            raise ValueError("sag_layer / sag_threshold / sag_blur_sigma without sag_scale > 0")
        return None
    if pag_scale_option(sk) > 0:
        raise ValueError("sag_scale with pag_scale: each forms the second half of the guided step its own way; stacking them "
                         "would need three evaluations")
    if cfg_distilled_option(sk):
        raise ValueError("sag_scale with cfg_distilled: a distilled student has one (conditional) evaluation per step, there "
                         "is no second half to guide with")
    if _opt(sk, "lv_native"):
        raise ValueError("sag_scale with the learned-variance 'native' update: the degraded image is formed from the mean "
                         "prediction alone; not implemented")
    if not fused or model is None:
        raise ValueError("sag_scale needs the fused step: the drop-in UNet's forward_with_cond_scale as denoise_sample_fn, no "
                         "p0 and no tensor cond_scale")
    if model.KIND == "unetca_fast":
        raise ValueError("self-attention guidance is not defined for unetca_fast: its Attention_LR keys are "
                         "[context | null | self], the map is not one over the image")
    if getattr(model, "use_spatial_transformer", False):
        raise ValueError("self-attention guidance is not implemented for use_spatial_transformer")
    layer, psi, sigma = (SAG_DEFAULTS[k] if v is None else v for k, v in given.items())
    known = model.attention_prefixes()
    if not isinstance(layer, str) or layer not in known:
        raise ValueError(f"sag_layer={layer!r}: one attention-layer prefix out of {known}")
    for name, v in (("sag_threshold", psi), ("sag_blur_sigma", sigma)):
        if not _real(v) or not 0.0 < v < float("inf"):
            raise ValueError(f"{name}={v!r}: a finite number > 0")
    if shape is not None and min(int(shape[-2]), int(shape[-1])) <= SAG_TAPS // 2:
        raise ValueError(f"sag_scale on a {int(shape[-2])}x{int(shape[-1])} image: the {SAG_TAPS}-tap blur reflects "
                         f"{SAG_TAPS // 2} pixels at the border, every side must be at least {SAG_TAPS // 2 + 1}")
    return s, layer, float(psi), float(sigma)


V_FORM_SAMPLERS = ("native", "ddim", "dpmsolver")


def _refuse_zero_snr(method, ac_visited):
    """ValueError for an eps-form trajectory that visits an ``alphas_cumprod`` of 0 (``ac_visited`` None: nothing to check)"""
    if ac_visited is not None and bool((np.asarray(ac_visited, dtype=np.float64) == 0.0).any()):
        raise ValueError(f"'{method}' on the eps form visits a time whose alphas_cumprod is 0 (a zero-terminal-SNR schedule): "
                         "x0 = (x - s1 eps) / sa is 0 / 0 there.  Use parameterization='v' with v_form='data' (native, ddim, "
                         "dpmsolver), or a timestep spacing that does not visit it")


def v_form_option(sk, method, ac_visited=None, par=None):
    """'eps' | 'data': the sampling kwarg ``v_form`` of a 'v' trajectory.  'eps' (default): the network output is changed to
    eps (sgd_v_to_eps) and the sampler's own kernel forms x0 = (x - s1 eps) / sa.  'data': ONE launch (sgd_v_step) forms
    x0 = sa x - s1 v and eps = sa v + s1 x and performs the update from them, finite at sa = 0.  ValueError, before anything
    is loaded or launched, for 'data' with a parameterization other than 'v' (``par``: the one in force when the kwargs leave
    it to the schedule), with dynamic thresholding, or on 'plms' / 'pndm' (multistep methods on eps; 'pndm' keeps a schedule of
    its own); and for an eps-form trajectory that visits an ``alphas_cumprod`` of 0 (``ac_visited``: the table entries of the
    visited times), where x0 = 0 / 0.  Pure host code: no device, no library."""
    sk = sk or {}
    form = _opt(sk, "v_form")
    if form not in ("eps", "data"):
        raise ValueError(f"v_form={form!r} ('eps' or 'data')")
    if form == "data":
        par = _opt(sk, "parameterization") if par is None else par
        if par != "v":
            raise ValueError(f"v_form='data' reads the network output as v: parameterization '{par}' has no data form")
        if _opt(sk, "dtp") < 1.0:
            raise ValueError("v_form='data': dynamic thresholding (dtp < 1) is not implemented on the data form")
        if method not in V_FORM_SAMPLERS:
            raise ValueError(f"v_form='data' is implemented for {', '.join(V_FORM_SAMPLERS)}; '{method}' is a multistep method "
                             "on eps")
    else:
        _refuse_zero_snr(method, ac_visited)
    return form


def native_steps_option(sk, method, T):
    """None | K: the sampling kwarg ``native_steps`` of the 'native' sampler, a strided ancestral chain over K of the T
    training times (2 <= K <= T).  ValueError, before anything is loaded or launched, on another sampler or out of range.
    Pure host code."""
    K = _opt(sk, "native_steps")
    if K is None:
        return None
    if method != "native":
        raise ValueError(f"native_steps strides the 'native' sampler; '{method}' takes num_timesteps")
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 2 <= K <= T:
        raise ValueError(f"native_steps={K!r}: an int, 2 .. {T}")
    return int(K)


LV_NATIVE_REFUSED = ("dtp", "noise_dropout", "cfg_interval", "cfg_rescale", "v_form")


def lv_native_option(sk):
    """the 'native' sampler of a learned-variance model (update kind 'lv_native', sgd_ddpm_lv_step) refuses what its one
    launch does not implement -- dynamic thresholding, noise dropout, the guidance schedule, the data form of 'v' (its row
    already avoids dividing by sqrt(alphas_cumprod) for 'v') -- with ValueError, before anything is loaded or launched"""
    sk = sk or {}
    if _opt(sk, "dtp") < 1.0:
        raise ValueError("learn_sigma 'native': dynamic thresholding (dtp < 1) is not implemented")
    if _opt(sk, "noise_dropout") > 0:
        raise ValueError("learn_sigma 'native': noise_dropout is not implemented")
    if _opt(sk, "cfg_interval") is not None or _opt(sk, "cfg_rescale") != 0:
        raise ValueError("learn_sigma 'native': cfg_interval / cfg_rescale are not implemented")
    if _opt(sk, "v_form") == "data":
        raise ValueError("learn_sigma 'native': v_form='data' is not needed, the row of a 'v' model never divides by "
                         "sqrt(alphas_cumprod)")


def cfg_schedule(times, cond_scale, scale_mode, interval=None):
    """per UNet EVALUATION of a trajectory (``times``: its time argument, one entry per evaluation -- PNDM's list repeats
    times): (guided, weight).  An evaluation is guided when ``t_lo <= t <= t_hi`` (``interval`` None: always) and then has
    weight ``cond_scale``; the others take the conditional prediction alone, which is weight 1 of the imagen form
    (``scale_mode`` 1, _scale_mode()) and weight 0 of the cfg form (2).  Pure host code."""
    if scale_mode not in (1, 2):
        raise ValueError(f"scale_mode={scale_mode!r} (1: imagen, 2: cfg)")
    off = 1.0 if scale_mode == 1 else 0.0
    guided = [interval is None or interval[0] <= int(t) <= interval[1] for t in times]
    return guided, [float(cond_scale) if g else off for g in guided]


def _fused(model, kw, distilled, pag_on):
    """whether a step takes the evaluation whose guided score is formed inside the step kernel: the drop-in UNet, a numeric
    guidance weight that is not the model kind's single-evaluation 0 / 1 shortcut, no ``p0``"""
    w = kw.get("cond_scale")
    if distilled:                                   # the same step with its conditional evaluation alone, whatever the weight
        return model is not None and kw.get("p0") is None
    if pag_on:                                      # PAG's doubled evaluation, SAG's pair, whatever the weight: cond_scale is not read
        return model is not None and kw.get("p0") is None and not isinstance(w, torch.Tensor)
    if model is None or not isinstance(w, (int, float)) or kw.get("p0") is not None:
        return False
    fast_int = isinstance(w, int) if model.KIND == "unetca_fast" else True
    return not (fast_int and w in (0, 1))


@dataclass(frozen=True)
class SamplingPlan:
    """one trajectory's options, frozen: what ``resolve_plan`` made of the sampling kwargs (defaults: ``DEFAULTS``)"""

    method: Optional[str]           # the sampler ('native', 'ddim', 'plms', 'pndm', 'dpmsolver'); None: a bare step runner
    # the parameterization in force (kwarg ``parameterization``; the schedule's own for a direct 'native' call) and, for 'v',
    # how the step reads the output (kwarg ``v_form``).  'eps': a v -> eps pass (sgd_v_to_eps) sits between the UNet and the
    # update.  'data': no such pass, the update (_VUpdate, sgd_v_step) reads v itself with the UNet's time and the two
    # schedule tables -- one launch fewer per evaluation, finite at sqrt(alphas_cumprod) = 0
    par: str
    form: str
    # the guidance schedule (kwargs ``cfg_rescale`` = phi, ``cfg_interval`` = (t_lo, t_hi)).  ``scheduled``: a guided evaluation
    # puts the guide pass (sgd_cfg_guide) behind the UNet and everything after it reads the guided buffer with mode 0, the
    # weight a device float; an evaluation outside the interval is ONE UNet evaluation at B, nothing dropped
    rescale: float
    interval: Optional[Tuple[int, int]]
    scheduled: bool
    # kwarg ``cfg_distilled`` (a guidance-distilled student): EVERY evaluation is the conditional one at B, cond_scale unread
    distilled: bool
    # kwargs ``pag_scale`` / ``pag_layers`` / ``pag_drop_cond`` (pag_options): None, or (s, layers, drop_cond) -- the doubled
    # evaluation runs on the perturbed-attention engine of ``layers`` and is read in the cfg form with weight s
    pag: Optional[tuple]
    # the learned-variance 'native' update: it reads the RAW 2C-wide output, both halves, whatever the parameterization.  Every
    # other update of such a model ignores the variance half (the engine's C-row head).  Known to the sampler, not a kwarg
    lv: bool
    native_steps: Optional[int]     # kwarg ``native_steps`` = K: the 'native' chain strided over K times
    dtp: float                      # kwarg ``dtp`` < 1: dynamic thresholding   } eager only, and only by an update
    noise_dropout: float            # kwarg ``noise_dropout``                  } that honours them (_Update.EXTRAS)
    clip: int                       # kwarg ``clip_denoised`` (no default), as the kernels take it; 'pndm': 0
    hip_graph: bool                 # kwarg ``hip_graph`` and SGDM_HIP_GRAPH != 0: the step may be captured
    fused: bool                     # the step kernels form the guided score from the engine's output (_fused)
    mode: Optional[int]             # fused: how they read a doubled evaluation -- the model's form; 2 (cfg) under PAG / SAG
    weight: Optional[float]         # fused: the weight of a guided evaluation -- cond_scale; pag_scale / sag_scale under PAG / SAG
    # kwargs ``sag_scale`` / ``sag_layer`` / ``sag_threshold`` / ``sag_blur_sigma`` (sag_options): None, or (s, layer, psi, sigma) --
    # a guided evaluation is TWO dependent evaluations at B, the second on the image degraded where ``layer`` attends, and the
    # pair is read in the cfg form with weight s
    sag: Optional[tuple] = None

    @property
    def layers(self):
        """the ``pag`` argument of the doubled evaluation's engine (UNetModelBase._engine): None without PAG"""
        return self.pag[1] if self.pag else None

    def schedule(self, times):
        """(guided flag, weight) per evaluation of a scheduled trajectory (cfg_schedule)"""
        return cfg_schedule(times, self.weight, self.mode, self.interval)

    def visits(self, ac_visited):
        """the ``alphas_cumprod`` of the visited times, for a sampler whose times follow from the plan ('native': native_steps;
        'dpmsolver': its table is built for the form): the refusal of v_form_option.  Returns the plan"""
        if self.form == "eps":
            _refuse_zero_snr(self.method, ac_visited)
        return self

    def captured(self, upd, capture=True):
        """whether the step of update ``upd`` is a captured one: the fused evaluation on the drop-in UNet and nothing asked of
        the update that only the eager step runs; ``capture`` False: the eps is the caller's (PLMS)"""
        return bool(capture and self.hip_graph and self.fused and upd.noise_dropout == 0 and upd.dtp >= 1.0)

    def capture_key(self):
        """what a captured step bakes in of the plan: two trajectories may share one capture only if these are equal.  A
        scheduled step reads its weight from the device, so a sweep over weights or intervals reuses one capture (whether
        an interval is requested stays: it adds the second graph); a static weight is a by-value kernel argument.  'v' on
        the eps form captures one more launch, the data form another update: three kinds.  PAG: the layer set chose the
        engine, ``drop_cond`` the mask's probabilities.  SAG: the layer names the tape buffers the capture reads, psi is a by-value
        argument and sigma the content of the captured step's own taps."""
        w = None if self.scheduled or self.distilled else self.weight
        kind = "eps" if self.lv or self.par != "v" else "v/" + self.form
        return (w, self.mode, kind, self.rescale, self.interval is not None, self.lv, self.distilled, self.pag and self.pag[1:],
                self.sag and self.sag[1:])


def resolve_plan(sk, method=None, model=None, denoise_kwargs=None, T=None, ac_visited=None, lv=False, par=None, shape=None):
    """the SamplingPlan of one trajectory, every refusal raised here: sampling kwargs ``sk``, the sampler's ``method`` name
    (None: a bare step runner, no sampler rules), the drop-in ``model`` behind the denoise function (None: a generic one), the
    denoise kwargs (``cond_scale``, ``p0``) and what only the sampler knows -- ``T`` training timesteps, ``ac_visited`` (the
    ``alphas_cumprod`` of the times it will visit; a sampler whose times follow from the plan calls ``plan.visits``), ``lv``
    (the learned-variance 'native' update), ``par`` (the schedule's parameterization, where the kwargs may leave it out) and ``shape``
    (the image's, for the one refusal that reads it: sag_options)."""
    sk, kw = sk or {}, denoise_kwargs or {}
    par = sk.get("parameterization", par or DEFAULTS["parameterization"])
    lv = bool(lv or _opt(sk, "lv_native"))
    K, form = None, "eps"
    if method is not None:
        K = native_steps_option(sk, method, T)
        if lv:
            lv_native_option(sk)
        form = v_form_option(sk, method, ac_visited, par)
    distilled = cfg_distilled_option(sk)
    fused = _fused(model, kw, distilled, pag_scale_option(sk) > 0 or sag_scale_option(sk) > 0)
    rescale, interval = cfg_options(dict(sk, lv_native=True) if lv else sk, fused)
    pag = pag_options(sk, fused, model)
    sag = sag_options(dict(sk, lv_native=True) if lv else sk, fused, model, shape)
    mode = weight = None
    if fused:
        mode = 2 if pag or sag else model._scale_mode()
        weight = (pag or sag)[0] if pag or sag else None if distilled else float(kw["cond_scale"])
    return SamplingPlan(
        method=method, par=par, form=form, rescale=rescale, interval=interval, scheduled=rescale > 0 or interval is not None,
        distilled=distilled, pag=pag, lv=lv, native_steps=K, dtp=_opt(sk, "dtp"), noise_dropout=_opt(sk, "noise_dropout"),
        clip=0 if method in (None, "pndm") else 1 if sk["clip_denoised"] else 0,       # (PNDM never clips; the others need it)
        hip_graph=bool(_opt(sk, "hip_graph")) and os.environ.get("SGDM_HIP_GRAPH", "1") != "0",
        fused=fused, mode=mode, weight=weight, sag=sag)
