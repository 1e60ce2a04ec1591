"""Drop-in diffusion process: ``diffusion.ddpm.LatentDiffusion`` and its samplers on the HIP path.

Mirrors (reference, /root/reference):
    diffusion/ddpm.py:24-126                      LatentDiffusion
    diffusion/sampler/ddpm_sampler.py:16-238      Schedule_DDPM   ('native' 1000-step ancestral sampler)
    diffusion/sampler/ddim_plms_sampler.py:25-391 DDIMSampler     ('ddim', 'plms')
    diffusion/sampler/pndm_sampler.py:13-211      PNDM_Sampler    ('pndm', include/sgdm_hip.h: sgd_pndm_step)
    dynamic/diffusionmodules/util.py:23-74        schedules / DDIM tables (deterministic host math)

Per sampling step the host issues: one UNet evaluation at 2B (cond | uncond halves, doubled inside
the boundary kernels) and ONE fused kernel doing CFG combine + x0 prediction + clip + posterior /
DDIM update + noise (include/sgdm_hip.h: sgd_ddpm_step / sgd_ddim_step).  RNG draws (x_T, the
per-step mask uniform_ and z) are kept in the reference's order so seeded runs line up.
"""
import copy
import ctypes as C
import os
import warnings
from functools import partial

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .unet import UNetModelBase, _cfg_eval, _ptr


class _Obj:
    """dict2obj (diffusion_utils/util.py:85-92)"""

    def __init__(self, d):
        for a, b in d.items():
            if isinstance(b, (list, tuple)):
                setattr(self, a, [_Obj(x) if isinstance(x, dict) else x for x in b])
            else:
                setattr(self, a, _Obj(b) if isinstance(b, dict) else b)


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    """util.py:23-43 (float64 host math, returned as numpy)"""
    if schedule == "linear":
        betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2
    elif schedule == "cosine":
        timesteps = torch.arange(n_timestep + 1, dtype=torch.float64) / n_timestep + cosine_s
        alphas = torch.cos(timesteps / (1 + cosine_s) * np.pi / 2).pow(2)
        alphas = alphas / alphas[0]
        betas = np.clip(1 - alphas[1:] / alphas[:-1], a_min=0, a_max=0.999)
    elif schedule == "sqrt_linear":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64)
    elif schedule == "sqrt":
        betas = torch.linspace(linear_start, linear_end, n_timestep, dtype=torch.float64) ** 0.5
    else:
        raise ValueError(f"schedule '{schedule}' unknown.")
    return betas.numpy()


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=False):
    """util.py:46-60"""
    if ddim_discr_method == "uniform":
        c = num_ddpm_timesteps // num_ddim_timesteps
        ddim_timesteps = np.asarray(list(range(0, num_ddpm_timesteps, c)))
    elif ddim_discr_method == "quad":
        ddim_timesteps = ((np.linspace(0, np.sqrt(num_ddpm_timesteps * .8), num_ddim_timesteps)) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    return ddim_timesteps + 1


def make_ddim_sampling_parameters(alphacums, ddim_timesteps, eta, verbose=False):
    """util.py:63-74 (alphacums: float32 CPU tensor, as the reference passes it)"""
    alphas = alphacums[ddim_timesteps]
    alphas_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist())
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - alphas) * (1 - alphas / alphas_prev))
    return sigmas, alphas, alphas_prev


def _unet_of(fn):
    """the drop-in UNet behind a bound ``forward_with_cond_scale`` (fast fused-CFG path), else None"""
    owner = getattr(fn, "__self__", None)
    if isinstance(owner, UNetModelBase) and getattr(fn, "__name__", "") == "forward_with_cond_scale":
        return owner
    return None


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _StepRunner:
    """one sampling step = UNet(2B) + one fused update kernel"""

    def __init__(self, denoise_sample_fn, kwargs):
        self.fn = denoise_sample_fn
        self.kwargs = dict(kwargs)
        self.model = _unet_of(getattr(denoise_sample_fn, "_sgdm_inner", denoise_sample_fn))
        self.lib = L.load()

    def eps(self, x, t):
        """returns (eps tensor/engine buffer, cfg_mode, w, b, c) describing how the step kernel reads it"""
        B, Cc = x.shape[0], x.shape[1]
        m = self.model
        if m is not None:
            w = self.kwargs.get("cond_scale")
            cond, layout = self.kwargs.get("cond"), self.kwargs.get("layout")
            fast_int = isinstance(w, int) if m.KIND == "unetca_fast" else isinstance(w, (int, float))
            if isinstance(w, (int, float)) and not (fast_int and w in (0, 1)) and self.kwargs.get("p0") is None:
                # batch-doubled evaluation, guided score formed inside the step kernel
                has_mask = (m._cond_width > 0) or (m._in_ch_total > m.in_channels)
                p = torch.cat((torch.full((B,), 0.0, device=x.device), torch.full((B,), 1.0, device=x.device)))
                mask = m._draw_mask(2 * B, p, x.device) if has_mask else None
                eng = m._run(x, t, cond, layout, mask, 2 * B)
                return eng.eps_nhwc, m._scale_mode(), float(w), B, Cc
        e = self.fn(x, t, **self.kwargs)            # generic path: guided eps, NCHW
        return e.contiguous(), 0, 0.0, B * Cc, 1


class _GraphedStep:
    """One CFG sampling step -- UNet at 2B (~135 launches) + the fused update -- captured into a hipGraph
    (``torch.cuda.CUDAGraph`` capture of the stream the C-ABI launchers are given), cached on the model per
    (batch, resolution, precision, guidance, sampler) and replayed per step.

    Everything a step varies lives in fixed device buffers the captured kernels read: ``img`` (updated in place by
    ``sgd_*_step_dev``), ``t`` [B], ``coef`` (row of the per-step table), ``z`` and the cond-drop mask.  The RNG draws
    (``z``, the mask's ``uniform_``) stay OUTSIDE the graph, in the reference's order, so seeded trajectories are the
    same with and without the graph.  Host work per step: 5 tiny torch ops + one graph launch instead of ~140 ctypes
    launches -- irrelevant at UNet batch 80 (21 ms of GPU work per step) and the difference between host-bound and
    device-bound at C1 size (ch=64, 32x32, bs=8).  Reference loops: ddpm_sampler.py:194-238, ddim_plms_sampler.py:302-344.
    """

    MAX_PER_ENGINE = 8          # captured steps kept per (model, batch, resolution, precision) engine

    @classmethod
    def get(cls, runner, img, kind, clip, temperature=1.0):
        """the captured step for this (model, batch, resolution, precision, guidance, sampler) -- built on first use and
        kept on the model, so later trajectories of the same configuration only refresh the static input buffers"""
        m, kw = runner.model, runner.kwargs
        cond, layout = kw.get("cond"), kw.get("layout")
        sig = lambda t: None if t is None else (tuple(t.shape), t.dtype)
        prec = L.PREC_BY_NAME[m.hip_precision]
        eng = m._engine(2 * img.shape[0], img.shape[2], img.shape[3], prec)
        key = (id(eng), tuple(img.shape), kind, clip, float(temperature), float(kw["cond_scale"]), m._scale_mode(),
               sig(cond), sig(layout))
        cache = m.__dict__.setdefault("_hip_graph_steps", {})
        g = cache.get(key)
        if g is None:
            live = {id(e) for e in m._engines.values()}
            for k in [k for k in cache if k[0] not in live]:
                del cache[k]                                # graphs of a replaced engine (parameters re-allocated)
            mine = [k for k in cache if k[0] == id(eng)]
            for k in mine[:max(0, len(mine) - (cls.MAX_PER_ENGINE - 1))]:
                del cache[k]                                # oldest first (dicts keep insertion order): a sweep over
                                                            # guidance weights / temperatures must not grow without bound
            g = cache[key] = cls(runner, eng, img, kind, clip, temperature)
        g.begin(img, cond, layout)
        return g

    def __init__(self, runner, eng, img, kind, clip, temperature=1.0):
        m = runner.model
        self.m, self.lib, self.kind, self.eng = m, runner.lib, kind, eng
        B, Cc = img.shape[0], img.shape[1]
        hw = int(np.prod(img.shape[2:]))
        dev = img.device
        self.img = torch.empty_like(img)
        self.t = torch.zeros(B, dtype=torch.long, device=dev)
        self.coef = torch.zeros(5, dtype=torch.float32, device=dev)
        self.z = torch.empty_like(img)
        self.x0 = torch.empty_like(img)                 # clipped x0 prediction of the step (snapshot steps clone it)
        kw = runner.kwargs
        # static copies in exactly the dtypes the boundary kernels read (prepare() must not re-allocate them)
        c0, l0 = kw.get("cond"), kw.get("layout")
        self.cond = None if c0 is None else (c0.detach().clone() if c0.dtype == torch.int64 else c0.detach().float().clone()).contiguous()
        self.layout = None if l0 is None else (l0.detach().clone() if l0.dtype in (torch.uint8, torch.int32, torch.int64)
                                               else l0.detach().float().clone()).contiguous()
        self.has_mask = (m._cond_width > 0) or (m._in_ch_total > m.in_channels)
        self.u = torch.zeros(2 * B, device=dev)
        self.p = torch.cat((torch.full((B,), 0.0, device=dev), torch.full((B,), 1.0, device=dev)))
        self.mask = torch.zeros(2 * B, dtype=torch.bool, device=dev)
        eng.prepare(self.img, self.t, self.cond, self.layout, self.mask if self.has_mask else None)
        self._inputs = eng._keep_inputs                 # the captured launches read these buffers on every replay
        img = self.img
        w, mode = float(kw["cond_scale"]), m._scale_mode()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            if not getattr(eng, "ran", False):
                eng.launch(side.cuda_stream)            # one-time function attributes are set outside the capture
            side.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side):
                st = torch.cuda.current_stream(dev).cuda_stream
                eng.launch(st)
                self._launch_update(st, img, mode, w, B, Cc, hw, kind, clip, temperature)
        torch.cuda.current_stream(dev).wait_stream(side)

    def _launch_update(self, st, img, mode, w, B, Cc, hw, kind, clip, temperature):
        """the update kernel of the captured step (reads the UNet's eps from the engine, updates img in place)"""
        eng = self.eng
        if kind == "ddpm":
            L.check(self.lib.sgd_ddpm_step_dev(_ptr(img), _ptr(eng.eps_nhwc), _ptr(self.z), mode, w, _ptr(self.coef),
                                               clip, B, Cc, hw, _ptr(img), _ptr(self.x0), st), "sgd_ddpm_step_dev")
        else:
            L.check(self.lib.sgd_ddim_step_dev(_ptr(img), _ptr(eng.eps_nhwc), _ptr(self.z), mode, w, _ptr(self.coef),
                                               float(temperature), clip, B, Cc, hw, _ptr(img), _ptr(self.x0), st),
                    "sgd_ddim_step_dev")

    def begin(self, img, cond, layout):
        """start of a trajectory: x_T and the guidance tensors into the static buffers; packed weights re-checked"""
        self.eng.refresh(torch.cuda.current_stream().cuda_stream)
        self.img.copy_(img)
        if self.cond is not None:
            self.cond.copy_(cond)
        if self.layout is not None:
            self.layout.copy_(layout)

    def step(self, t_row, coef_row, noise=None):
        """t_row: [B] long device tensor; coef_row: device tensor [5]; draws the mask uniform and z like the eager path"""
        if self.has_mask:
            self.u.uniform_(0, 1)                       # prob_mask_like (openaimodel.py:462-463): same RNG consumption
            torch.lt(self.u, self.p, out=self.mask)
        self.t.copy_(t_row)
        if noise is None:
            self.z.normal_()                            # == torch.randn(shape) (noise_like, util.py:264-267)
        else:
            self.z.copy_(noise)
        self.coef.copy_(coef_row)
        self.graph.replay()


class _GraphedPNDMStep(_GraphedStep):
    """The captured step of the PNDM sampler: UNet at 2B + ``sgd_pndm_step``.  Its static buffers are the Runge-Kutta
    accumulator, the warm-up start image and the 3-slot eps history; ``row`` (include/sgdm_hip.h: sgd_pndm_row) says which
    update the replay performs, so ONE graph serves warm-up and multistep evaluations alike.  No ``z`` is drawn: the only
    RNG use per evaluation is the cond-drop mask's ``uniform_``, as in the reference (pndm_sampler.py:176-208)."""

    def __init__(self, runner, eng, img, kind, clip, temperature=1.0):
        self.acc = torch.empty_like(img)
        self.base = torch.empty_like(img)
        self.ring = torch.empty((3,) + tuple(img.shape), dtype=img.dtype, device=img.device)
        self.row = torch.zeros(8, dtype=torch.int32, device=img.device)
        super().__init__(runner, eng, img, kind, clip, temperature)

    def _launch_update(self, st, img, mode, w, B, Cc, hw, kind, clip, temperature):
        L.check(self.lib.sgd_pndm_step(_ptr(img), _ptr(self.eng.eps_nhwc), mode, w, _ptr(self.row), _ptr(self.acc),
                                       _ptr(self.base), _ptr(self.ring), B, Cc, hw, _ptr(img), st), "sgd_pndm_step")

    def step(self, t_row, row):
        """t_row: [B] long device tensor; row: [8] int32 device tensor (one sgd_pndm_row)"""
        if self.has_mask:
            self.u.uniform_(0, 1)                       # prob_mask_like: the eager path's only draw per evaluation
            torch.lt(self.u, self.p, out=self.mask)
        self.t.copy_(t_row)
        self.row.copy_(row)
        self.graph.replay()


def _graph_ok(runner, sk, kwargs):
    """the captured step covers the common case only: fused CFG evaluation on the drop-in UNet, a numeric guidance weight,
    no noise dropout, no dynamic thresholding; ``hip_graph=False`` in the sampling kwargs turns it off"""
    m = runner.model
    w = runner.kwargs.get("cond_scale")
    if m is None or not sk.get("hip_graph", True) or os.environ.get("SGDM_HIP_GRAPH", "1") == "0":
        return False
    fast_int = isinstance(w, int) if m.KIND == "unetca_fast" else isinstance(w, (int, float))
    if not isinstance(w, (int, float)) or (fast_int and w in (0, 1)) or runner.kwargs.get("p0") is not None:
        return False
    return sk.get("noise_dropout", 0) == 0 and sk.get("dtp", 1) >= 1.0


def _quantile_rank(dtp, count):
    """(lo, hi, frac) of torch.quantile(., dtp) over `count` fp32 values: rank = q * (count - 1) in the input dtype,
    linear interpolation between the order statistics floor(rank) and ceil(rank)"""
    rank = torch.tensor(dtp, dtype=torch.float32) * (count - 1)
    lo = torch.floor(rank)
    return int(lo), int(torch.ceil(rank)), float(rank - lo)


class Schedule_DDPM(nn.Module):
    """ddpm_sampler.py:16-238"""

    def __init__(self, **kwargs):
        super().__init__()
        self.hparams = _Obj(kwargs)
        h = self.hparams
        self.register_schedule(given_betas=h.given_betas, beta_schedule=h.beta_schedule, timesteps=h.num_timesteps,
                               linear_start=h.linear_start, linear_end=h.linear_end, cosine_s=h.cosine_s)

    def register_schedule(self, given_betas=None, beta_schedule="linear", timesteps=1000, linear_start=1e-4,
                          linear_end=2e-2, cosine_s=8e-3):
        h = self.hparams
        key = (id(given_betas) if given_betas is not None else None, beta_schedule, timesteps, linear_start,
               linear_end, cosine_s)
        if getattr(self, "_sched_key", None) == key:
            return                       # the reference rebuilds identical buffers on every sample() call
        betas = given_betas if given_betas is not None else make_beta_schedule(
            beta_schedule, h.num_timesteps, linear_start=linear_start, linear_end=linear_end, cosine_s=cosine_s)
        alphas = 1. - betas
        alphas_cumprod = np.cumprod(alphas, axis=0)
        alphas_cumprod_prev = np.append(1., alphas_cumprod[:-1])
        if timesteps < h.num_timesteps:
            raise NotImplementedError                      # ddpm_sampler.py:38-39
        self.linear_start, self.linear_end = linear_start, linear_end
        assert alphas_cumprod.shape[0] == timesteps, "alphas have to be defined for each timestep"
        dev = h.device
        to_torch = lambda a: torch.tensor(a, dtype=torch.float32).to(dev)
        reg = self.register_buffer
        reg("betas", to_torch(betas))
        reg("alphas_cumprod", to_torch(alphas_cumprod))
        reg("alphas_cumprod_prev", to_torch(alphas_cumprod_prev))
        reg("sqrt_alphas_cumprod", to_torch(np.sqrt(alphas_cumprod)))
        reg("sqrt_one_minus_alphas_cumprod", to_torch(np.sqrt(1. - alphas_cumprod)))
        reg("log_one_minus_alphas_cumprod", to_torch(np.log(1. - alphas_cumprod)))
        reg("sqrt_recip_alphas_cumprod", to_torch(np.sqrt(1. / alphas_cumprod)))
        reg("sqrt_recipm1_alphas_cumprod", to_torch(np.sqrt(1. / alphas_cumprod - 1)))
        vp = h.v_posterior
        posterior_variance = (1 - vp) * betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod) + vp * betas
        reg("posterior_variance", to_torch(posterior_variance))
        reg("posterior_log_variance_clipped", to_torch(np.log(np.maximum(posterior_variance, 1e-20))))
        reg("posterior_mean_coef1", to_torch(betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod)))
        reg("posterior_mean_coef2", to_torch((1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod)))
        if h.parameterization == "eps":
            lvlb = self.betas ** 2 / (2 * self.posterior_variance * to_torch(alphas) * (1 - self.alphas_cumprod))
        elif h.parameterization == "x0":
            lvlb = (0.5 * np.sqrt(torch.Tensor(alphas_cumprod)) / (2. * 1 - torch.Tensor(alphas_cumprod))).to(dev)
        else:
            raise NotImplementedError("mu not supported")
        lvlb[0] = lvlb[1]
        reg("lvlb_weights", lvlb, persistent=False)
        assert not torch.isnan(self.lvlb_weights).all()
        reg("snr_derivative", torch.zeros(1000, dtype=torch.float32).to(dev))
        reg("SNR", torch.zeros(1000, dtype=torch.float32).to(dev))
        # host copies of the per-step scalars of the fused step kernel (fp32 math as on the device)
        f = lambda name: getattr(self, name).detach().cpu()
        self._step_tab = torch.stack([f("sqrt_recip_alphas_cumprod"), f("sqrt_recipm1_alphas_cumprod"),
                                      f("posterior_mean_coef1"), f("posterior_mean_coef2"),
                                      (0.5 * f("posterior_log_variance_clipped")).exp()], 1).contiguous()
        self._sched_key = key

    @staticmethod
    def _ext(a, t, x_shape):
        return a.gather(-1, t).reshape(t.shape[0], *((1,) * (len(x_shape) - 1)))

    def q_sample(self, original_sample, noise, t):
        noise = torch.randn_like(original_sample) if noise is None else noise
        return (self._ext(self.sqrt_alphas_cumprod, t, original_sample.shape) * original_sample
                + self._ext(self.sqrt_one_minus_alphas_cumprod, t, original_sample.shape) * noise)

    def predict_start_from_noise(self, x_t, t, noise):
        return (self._ext(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - self._ext(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, original_sample, x_t, t):
        mean = (self._ext(self.posterior_mean_coef1, t, x_t.shape) * original_sample
                + self._ext(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return (mean, self._ext(self.posterior_variance, t, x_t.shape),
                self._ext(self.posterior_log_variance_clipped, t, x_t.shape))

    def vis_schedule(self):
        try:
            from diffusion_utils.taokit.wandb_utils import vis_schedule_ddpm     # the reference's wandb helper
        except Exception:
            return {}
        return vis_schedule_ddpm(_betas=self.betas.cpu(), _alphas_cumprod=self.alphas_cumprod.cpu(), _snr_derivative=None)

    @torch.no_grad()
    def sample(self, shape, sampling_kwargs=None, denoise_sample_fn=None, denoise_sample_fn_kwargs=None, **kwargs):
        """ancestral DDPM loop (ddpm_sampler.py:194-238); ``x_T`` / ``noise_fn(i)`` may be injected for tests"""
        sk = sampling_kwargs
        temperature, noise_dropout = sk["temperature"], sk["noise_dropout"]
        timesteps = sk["num_timesteps"]
        h = self.hparams
        self.register_schedule(timesteps=timesteps, given_betas=h.given_betas, beta_schedule=h.beta_schedule,
                               linear_start=h.linear_start, linear_end=h.linear_end, cosine_s=h.cosine_s)
        dyn = sk.get("dtp", 1) < 1.0            # dynamic thresholding (diffusion_utils/util.py:70-79)
        if h.parameterization not in ("eps", "x0"):
            raise NotImplementedError()                                        # ddpm_sampler.py:162-163
        x0_param = h.parameterization == "x0"
        dev = self.betas.device
        B, Cc = shape[0], shape[1]
        hw = int(np.prod(shape[2:]))
        x_T = kwargs.get("x_T")
        img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev).float().contiguous()
        noise_fn = kwargs.get("noise_fn")
        if type(temperature) == float or isinstance(temperature, int):
            temperature = [float(temperature)] * timesteps
        snaps = torch.linspace(0, timesteps, sk["log_num_per_prog"], dtype=torch.int).cpu().numpy().tolist()
        runner = _StepRunner(denoise_sample_fn, denoise_sample_fn_kwargs or {})
        lib = runner.lib
        ts_tab = torch.arange(timesteps, device=dev, dtype=torch.long).view(-1, 1).expand(timesteps, B).contiguous()
        pred, inter = [], []
        clip = 1 if sk["clip_denoised"] else 0
        coef = (C.c_float * 5)()
        nxt = torch.empty_like(img)
        order = kwargs.get("step_indices")          # bench / teacher-forced tests: visit only these steps
        order = list(reversed(range(0, timesteps))) if order is None else list(order)
        gstep, coef_dev = None, None
        if _graph_ok(runner, sk, kwargs):
            tab = self._step_tab.double()                                       # same double product -> fp32 as below
            if x0_param:
                tab[:, 0], tab[:, 1] = 0.0, -1.0
            tab[:, 4] *= torch.tensor([float(v) for v in temperature], dtype=torch.float64)
            tab[0, 4] = 0.0                                                     # no noise when t == 0
            coef_dev = tab.float().to(dev)
            gstep = _GraphedStep.get(runner, img, "ddpm", clip)
            img = gstep.img                                                     # updated in place by the replays
        for i in order:
            ts = ts_tab[i]
            want = i in snaps
            if gstep is not None:
                gstep.step(ts, coef_dev[i], None if noise_fn is None else noise_fn(i).to(dev))
                if want:
                    pred.append(gstep.x0.clone().unsqueeze(0))
                    inter.append(img.clone().unsqueeze(0))
                continue
            eps, mode, w, bb, cc = runner.eps(img, ts)
            z = torch.randn(shape, device=dev) if noise_fn is None else noise_fn(i).to(dev)
            if noise_dropout > 0.:
                z = torch.nn.functional.dropout(z, p=noise_dropout)
            row = self._step_tab[i]
            coef[0], coef[1], coef[2], coef[3] = row[0], row[1], row[2], row[3]
            if x0_param:
                coef[0], coef[1] = 0.0, -1.0        # x_recon = model_out (ddpm_sampler.py:160-161): 0*x - (-1)*out, exact
            coef[4] = (float(row[4]) * float(temperature[i])) if i != 0 else 0.0      # no noise when t == 0
            x0 = torch.empty_like(img) if want else None
            if dyn:
                lo, hi, frac = _quantile_rank(sk["dtp"], Cc * hw)
                s_dyn = torch.empty(B, device=dev)
                # the step kernels see a guided NCHW eps as (B*C) one-channel planes; the quantile is per SAMPLE
                e4 = eps if mode else eps.reshape(B, Cc, hw).permute(0, 2, 1).contiguous()
                L.check(lib.sgd_x0_quantile(0, _ptr(img), _ptr(e4), mode, w, coef, B, Cc, hw, lo, hi, frac, _ptr(s_dyn),
                                            _stream()), "sgd_x0_quantile")
                L.check(lib.sgd_ddpm_step_dyn(_ptr(img), _ptr(e4), _ptr(z), mode, w, coef, _ptr(s_dyn), B, Cc, hw,
                                              _ptr(nxt), _ptr(x0), _stream()), "sgd_ddpm_step_dyn")
            else:
                L.check(lib.sgd_ddpm_step(_ptr(img), _ptr(eps), _ptr(z), mode, w, coef, clip, bb, cc, hw,
                                          _ptr(nxt), _ptr(x0), _stream()), "sgd_ddpm_step")
            img, nxt = nxt, img
            if want:
                pred.append(x0.unsqueeze(0))
                inter.append(img.clone().unsqueeze(0))
        if gstep is not None:
            img = img.clone()                       # the static buffer belongs to the cached graph
        if not pred:
            return img, dict(pred_x0=img.new_zeros((0,) + tuple(shape)), x_inter=img.new_zeros((0,) + tuple(shape)))
        return img, dict(pred_x0=torch.cat(pred, 0), x_inter=torch.cat(inter, 0))


class DDIMSampler(object):
    """ddim_plms_sampler.py:25-525 (sampler_type 'ddim' | 'plms')"""

    def __init__(self, ddpm_num_timesteps, device, sampler_type):
        self.ddpm_num_timesteps = ddpm_num_timesteps
        self.device = device
        self.sampler_type = sampler_type

    def make_schedule(self, sampling_kwargs, ddim_discretize="uniform", **kwargs):
        S, eta = sampling_kwargs["num_timesteps"], sampling_kwargs["ddim_eta"]
        if eta != 0 and self.sampler_type == "plms":
            eta = 0                                               # ddim_plms_sampler.py:41-45 (warns and resets)
        ac = sampling_kwargs["alphas_cumprod"]
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, S, self.ddpm_num_timesteps)
        assert ac.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        sig, a, ap = make_ddim_sampling_parameters(ac.detach().float().cpu(), self.ddim_timesteps, eta)
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = sig, a, ap
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1.0 - a)

    @torch.no_grad()
    def sample(self, shape, sampling_kwargs=None, **kwargs):
        self.make_schedule(sampling_kwargs=sampling_kwargs)
        if self.sampler_type == "ddim":
            return self.ddim_sampling(shape, sampling_kwargs=sampling_kwargs, **kwargs)
        if self.sampler_type == "plms":
            return self.plms_sampling(shape, sampling_kwargs=sampling_kwargs, **kwargs)
        raise NotImplementedError

    @torch.no_grad()
    def plms_sampling(self, shape, sampling_kwargs, denoise_sample_fn_kwargs=None, denoise_sample_fn=None, **kwargs):
        """ddim_plms_sampler.py:394-482: pseudo linear multistep.  Per step ONE UNet evaluation at 2B (two on the
        first step), the guided eps kept as a [B,3,H,W] tensor for the Adams-Bashforth history, and the same fused
        update kernel as DDIM (p_sample_plms == p_sample_ddim with a given eps, ddim_plms_sampler.py:484-525).
        RNG order of the reference: x_T, then one randn per p_sample_plms call (num_steps + 1 draws)."""
        sk = sampling_kwargs
        dyn = sk.get("dtp", 1) < 1.0                             # ddim_plms_sampler.py:505-512 (same helper as ddim)
        dev = torch.device(self.device)
        B, Cc = shape[0], shape[1]
        hw = int(np.prod(shape[2:]))
        x_T = kwargs.get("x_T")
        img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev).float().contiguous()
        noise_fn = kwargs.get("noise_fn")
        timesteps = self.ddim_timesteps
        total = timesteps.shape[0]
        time_range = np.flip(timesteps)
        snaps = torch.linspace(0, total, sk["log_num_per_prog"], dtype=torch.int).cpu().numpy().tolist()
        runner = _StepRunner(denoise_sample_fn, denoise_sample_fn_kwargs or {})
        lib = runner.lib
        clip = 1 if sk["clip_denoised"] else 0
        coef = (C.c_float * 4)()
        draws = [0]

        def guided(x, ts):
            eps, mode, w, bb, cc = runner.eps(x, ts)
            if mode == 0:
                return eps.reshape(shape).clone()
            out = torch.empty(shape, device=dev)
            L.check(lib.sgd_cfg_combine(_ptr(eps), mode, w, bb, cc, hw, _ptr(out), _stream()), "sgd_cfg_combine")
            return out

        def update(x, e, index, want_x0):
            z = torch.randn(shape, device=dev) if noise_fn is None else noise_fn(draws[0]).to(dev)
            draws[0] += 1
            if sk["noise_dropout"] > 0.0:
                z = torch.nn.functional.dropout(z, p=sk["noise_dropout"])
            coef[0] = float(self.ddim_sqrt_one_minus_alphas[index])
            coef[1] = float(self.ddim_alphas[index])
            coef[2] = float(self.ddim_alphas_prev[index])
            coef[3] = float(self.ddim_sigmas[index])
            nxt = torch.empty_like(x)
            x0 = torch.empty_like(x) if want_x0 else None
            if dyn:
                lo, hi, frac = _quantile_rank(sk["dtp"], Cc * hw)
                s_dyn = torch.empty(B, device=dev)
                e4 = e.reshape(B, Cc, hw).permute(0, 2, 1).contiguous()
                L.check(lib.sgd_x0_quantile(1, _ptr(x), _ptr(e4), 0, 0.0, coef, B, Cc, hw, lo, hi, frac, _ptr(s_dyn),
                                            _stream()), "sgd_x0_quantile")
                L.check(lib.sgd_ddim_step_dyn(_ptr(x), _ptr(e4), _ptr(z), 0, 0.0, coef, float(sk["temperature"]),
                                              _ptr(s_dyn), B, Cc, hw, _ptr(nxt), _ptr(x0), _stream()), "sgd_ddim_step_dyn")
                return nxt, x0
            e = e.contiguous()
            # a guided NCHW eps is "NHWC with one channel" over B*C planes
            L.check(lib.sgd_ddim_step(_ptr(x), _ptr(e), _ptr(z), 0, 0.0, coef, float(sk["temperature"]), clip,
                                      B * Cc, 1, hw, _ptr(nxt), _ptr(x0), _stream()), "sgd_ddim_step")
            return nxt, x0

        old_eps, pred, inter = [], [], []
        for i, step in enumerate(time_range):
            index = total - i - 1
            ts = torch.full((B,), int(step), device=dev, dtype=torch.long)
            e_t = guided(img, ts)
            if len(old_eps) == 0:
                ts_next = torch.full((B,), int(time_range[min(i + 1, len(time_range) - 1)]), device=dev, dtype=torch.long)
                x_prev, _ = update(img, e_t, index, False)
                e_t_prime = (e_t + guided(x_prev, ts_next)) / 2
            elif len(old_eps) == 1:
                e_t_prime = (3 * e_t - old_eps[-1]) / 2
            elif len(old_eps) == 2:
                e_t_prime = (23 * e_t - 16 * old_eps[-1] + 5 * old_eps[-2]) / 12
            else:
                e_t_prime = (55 * e_t - 59 * old_eps[-1] + 37 * old_eps[-2] - 9 * old_eps[-3]) / 24
            want = index in snaps
            img, x0 = update(img, e_t_prime, index, want)
            old_eps.append(e_t)
            if len(old_eps) >= 4:
                old_eps.pop(0)
            if want:
                inter.append(img.unsqueeze(0))
                pred.append(x0.unsqueeze(0))
        return img, dict(x_inter=torch.cat(inter, 0), pred_x0=torch.cat(pred, 0))

    @torch.no_grad()
    def ddim_sampling(self, shape, sampling_kwargs, denoise_sample_fn_kwargs=None, denoise_sample_fn=None, **kwargs):
        sk = sampling_kwargs
        dyn = sk.get("dtp", 1) < 1.0
        dev = torch.device(self.device)
        x_T = kwargs.get("x_T")
        img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev).float().contiguous()
        dkw = dict(denoise_sample_fn_kwargs or {})
        vis = sk.get("vis")
        vis_noise = kwargs.get("vis_noise")                     # tests: the start noise a `vis` branch would draw

        def vis_randn(sh):
            if vis_noise is None:
                return torch.randn(sh, device=dev)
            assert tuple(vis_noise.shape) == tuple(sh), (tuple(vis_noise.shape), tuple(sh))
            return vis_noise.to(dev).float()

        def should_vis(name):                                   # eval/test_exps/common_stuff.py:35-36
            return vis is not None and hasattr(vis, name) and bool(getattr(vis, name))

        if should_vis("scoremix_vis"):
            raise NotImplementedError                           # the reference raises here too (ddim_plms_sampler.py:177-178)
        if should_vis("interp"):
            # guidance interpolation strips (ddim_plms_sampler.py:142-155): `samples` pairs of neighbouring conds, `n` slerp
            # points each, ONE start noise shared by the whole batch; the float cond rows go through the UNet unchanged
            from .util import batch_to_conditioninterp
            dkw["cond"] = batch_to_conditioninterp(dkw["cond"], interp_num=vis.interp_c.n, samples=vis.interp_c.samples)
            img = vis_randn(list(shape[1:])).unsqueeze(0).repeat(len(dkw["cond"]), 1, 1, 1).contiguous()
        if should_vis("condscale"):
            # guidance-weight sweep (ddim_plms_sampler.py:107-140): `samples` start noises x 8 weights 0, 3/8, .. 21/8,
            # per-sample tensor cond_scale; only the `layout` entry of the kwargs is re-batched, as in the reference
            ns, nw = vis.condscale_c.samples, 8
            scales = [i * 3.0 / nw for i in range(nw)]
            cs = torch.tensor(scales * ns, device=dev).reshape(-1, 1, 1, 1)
            img = vis_randn([ns] + list(shape[1:])).repeat_interleave(nw, 0)
            assert len(dkw["layout"]) >= ns
            dkw["layout"] = dkw["layout"][:ns].repeat_interleave(nw, 0)
            assert len(cs) == len(img) == len(dkw["layout"])
            dkw["cond_scale"] = cs
        if should_vis("chainvis"):
            # conditional / unconditional chain pairs from the same start noise (ddim_plms_sampler.py:157-175)
            ns = vis.chainvis_c.samples
            img = vis_randn([ns] + list(shape[1:])).repeat_interleave(2, 0)
            dkw["cond"] = dkw["cond"][:ns].repeat_interleave(2, 0)
            assert len(dkw["cond"]) == len(img)
            dkw["p0"] = torch.tensor([1, 0], device=dev, dtype=torch.float32).repeat(ns)
        denoise_sample_fn_kwargs = dkw
        shape = tuple(img.shape)
        B, Cc = shape[0], shape[1]
        hw = int(np.prod(shape[2:]))
        noise_fn = kwargs.get("noise_fn")
        timesteps = self.ddim_timesteps
        total = timesteps.shape[0]
        snaps = torch.linspace(0, total, sk["log_num_per_prog"], dtype=torch.int).cpu().numpy().tolist()
        runner = _StepRunner(denoise_sample_fn, denoise_sample_fn_kwargs or {})
        lib = runner.lib
        pred, inter = [], []
        clip = 1 if sk["clip_denoised"] else 0
        coef = (C.c_float * 4)()
        nxt = torch.empty_like(img)
        gstep, coef_dev = None, None
        if _graph_ok(runner, sk, kwargs):
            tab = np.stack([self.ddim_sqrt_one_minus_alphas, self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sigmas,
                            np.zeros_like(self.ddim_sigmas)], 1)
            coef_dev = torch.tensor(tab, dtype=torch.float64).float().to(dev)   # float(table[index]) -> fp32, as below
            gstep = _GraphedStep.get(runner, img, "ddim", clip, temperature=float(sk["temperature"]))
            img = gstep.img
            ts_dev = torch.tensor(np.ascontiguousarray(timesteps), dtype=torch.long, device=dev).view(-1, 1).expand(total, B).contiguous()
        # step_indices (teacher-forced tests): visit only these table indices, in the order given
        visit = kwargs.get("step_indices")
        walk = list(enumerate(np.flip(timesteps))) if visit is None else [(total - int(ix) - 1, timesteps[int(ix)]) for ix in visit]
        for i, step in walk:
            index = total - i - 1
            want = index in snaps
            if gstep is not None:
                gstep.step(ts_dev[index], coef_dev[index], None if noise_fn is None else noise_fn(i).to(dev))
                if want:
                    inter.append(img.detach().cpu().unsqueeze(0))
                    pred.append(gstep.x0.detach().cpu().unsqueeze(0))
                continue
            ts = torch.full((B,), int(step), device=dev, dtype=torch.long)
            eps, mode, w, bb, cc = runner.eps(img, ts)
            z = torch.randn(shape, device=dev) if noise_fn is None else noise_fn(i).to(dev)    # drawn even at eta=0
            if sk["noise_dropout"] > 0.0:
                z = torch.nn.functional.dropout(z, p=sk["noise_dropout"])
            # torch.full_like(x, table[index]) casts the table entry to fp32 (ddim_plms_sampler.py:360-366)
            coef[0] = float(self.ddim_sqrt_one_minus_alphas[index])
            coef[1] = float(self.ddim_alphas[index])
            coef[2] = float(self.ddim_alphas_prev[index])
            coef[3] = float(self.ddim_sigmas[index])
            x0 = torch.empty_like(img) if want else None
            if dyn:
                lo, hi, frac = _quantile_rank(sk["dtp"], Cc * hw)
                s_dyn = torch.empty(B, device=dev)
                e4 = eps if mode else eps.reshape(B, Cc, hw).permute(0, 2, 1).contiguous()
                L.check(lib.sgd_x0_quantile(1, _ptr(img), _ptr(e4), mode, w, coef, B, Cc, hw, lo, hi, frac, _ptr(s_dyn),
                                            _stream()), "sgd_x0_quantile")
                L.check(lib.sgd_ddim_step_dyn(_ptr(img), _ptr(e4), _ptr(z), mode, w, coef, float(sk["temperature"]),
                                              _ptr(s_dyn), B, Cc, hw, _ptr(nxt), _ptr(x0), _stream()), "sgd_ddim_step_dyn")
            else:
                L.check(lib.sgd_ddim_step(_ptr(img), _ptr(eps), _ptr(z), mode, w, coef, float(sk["temperature"]), clip,
                                          bb, cc, hw, _ptr(nxt), _ptr(x0), _stream()), "sgd_ddim_step")
            img, nxt = nxt, img
            if want:
                inter.append(img.detach().cpu().unsqueeze(0))
                pred.append(x0.detach().cpu().unsqueeze(0))
        if gstep is not None:
            img = img.clone()                       # the static buffer belongs to the cached graph
        if not pred:
            return img, dict(x_inter=img.new_zeros((0,) + tuple(shape)).cpu(), pred_x0=img.new_zeros((0,) + tuple(shape)).cpu())
        return img, dict(x_inter=torch.cat(inter, 0), pred_x0=torch.cat(pred, 0))


PNDM_RK0, PNDM_RK12, PNDM_RK3, PNDM_PLMS = 0, 1, 2, 3            # include/sgdm_hip.h: SGD_PNDM_*


class PNDM_Sampler(object):
    """pndm_sampler.py:147-211 with its PNDMScheduler (:13-145): F-PNDM, 12 Runge-Kutta warm-up evaluations then one
    4th-order linear multistep evaluation per time.  Per evaluation ONE UNet call (at 2B on the fused-CFG path) and ONE
    ``sgd_pndm_step`` launch; the per-evaluation scalars form a table uploaded once per trajectory (``plan``).

    Kept from the reference: its own schedule (fp32 linear betas whatever the model's ``beta_schedule``, a trailing 0.0 so
    that every lookup reads ``alphas_cumprod[t + 1]``); no clipping and no noise after ``x_T`` (``clip_denoised``, ``dtp``,
    ``temperature``, ``noise_dropout`` and ``vis`` are ignored); the last multistep evaluation (t = t_next = 0) is a no-op
    update but is still evaluated; the return value ``(image, dict(pred_x0=image))``.  Tests may inject ``x_T=``.
    Step counts whose inference times include 999 (n = 3, 9, 27, 36-37, 101-111, 251-333, 501-1000) start the warm-up at the
    appended alphas_cumprod[1000] = 0.0: the reference's transfer divides by zero there, and the same infinite scalars go
    into the table here unchanged."""

    def __init__(self, ddpm_num_timesteps, beta_start, beta_end, beta_schedule="linear", tensor_format="pt", device="cuda"):
        self.ddpm_num_timesteps = ddpm_num_timesteps
        self.device = device
        self.beta_start, self.beta_end = beta_start, beta_end
        self.beta_schedule = beta_schedule          # stored only: the reference's scheduler is always built linear
        self.tensor_format = tensor_format
        # pndm_sampler.py:31-45 (PNDMScheduler(timesteps, beta_start, beta_end) with its default beta_schedule)
        betas = np.linspace(beta_start, beta_end, ddpm_num_timesteps, dtype=np.float32)
        alphas_cumprod = np.cumprod(1.0 - betas, axis=0)
        self.alphas_cumprod = torch.from_numpy(np.array(list(alphas_cumprod) + [0.0], dtype=np.float32))

    def time_steps(self, num_inference_steps):
        """(warm-up times, multistep times) of pndm_sampler.py:74-94.  ValueError where the reference fails with one:
        fewer than four inference times (numpy broadcast) or num_inference_steps > ddpm_num_timesteps (range step 0)."""
        T, n = self.ddpm_num_timesteps, int(num_inference_steps)
        step = T // n
        if step == 0:
            raise ValueError(f"PNDM: num_timesteps={n} > {T} gives a time step of 0")
        times = list(range(0, T, step))
        if len(times) < 4:
            raise ValueError(f"PNDM: num_timesteps={n} gives {len(times)} inference times; the warm-up needs 4")
        last = np.array(times[-4:]).repeat(2) + np.tile(np.array([0, step // 2]), 4)
        warmup = [int(v) for v in reversed(last[:-1].repeat(2)[1:-1])]
        return warmup, list(reversed(times[:-3]))

    def plan(self, num_inference_steps):
        """(UNet time per evaluation, [E, 8] int32 table of sgd_pndm_row).  The transfer scalars are the reference's fp32
        expressions (pndm_sampler.py:128-141) in IEEE fp32 arithmetic -- numpy float32, whose sqrt and divide are correctly
        rounded on every host.  (torch's CPU sqrt is not: it differs from the correctly rounded value for ~14 % of fp32
        inputs, by an amount that depends on the host CPU, so a table built with it would not be the same table on every
        machine.  The reference on the GPU, its configured device, rounds sqrt and divide correctly, as here.)"""
        warmup, plms = self.time_steps(num_inference_steps)
        ev = []                                     # (t, t_prev, t_next, phase, slot1, slot2, slot3)
        for j, t in enumerate(warmup):              # step_prk (:96-115)
            ev.append((t, warmup[j // 4 * 4], warmup[min(j + 1, len(warmup) - 1)], (PNDM_RK0, PNDM_RK12, PNDM_RK12, PNDM_RK3)[j % 4],
                       j // 4, 0, 0))
        for k, t in enumerate(plms):                # step_plms (:117-126): ets[-2], ets[-3], ets[-4] in ring slots
            ev.append((t, t, plms[min(k + 1, len(plms) - 1)], PNDM_PLMS, (k + 2) % 3, (k + 1) % 3, k % 3))
        ac = self.alphas_cumprod.numpy()
        at = ac[[e[1] + 1 for e in ev]]
        at_next = ac[[e[2] + 1 for e in ev]]
        one = np.float32(1)
        with np.errstate(divide="ignore", invalid="ignore"):        # t = 999 reads the appended 0.0 (class docstring)
            d = at_next - at
            c1 = one / (np.sqrt(at) * (np.sqrt(at) + np.sqrt(at_next)))
            c2 = one / (np.sqrt(at) * (np.sqrt((one - at_next) * at) + np.sqrt((one - at) * at_next)))
        tab = torch.zeros(len(ev), 8, dtype=torch.int32)
        tab[:, 0:3] = torch.from_numpy(np.ascontiguousarray(np.stack([d, c1, c2], 1), dtype=np.float32)).view(torch.int32)
        tab[:, 4:8] = torch.tensor([e[3:] for e in ev], dtype=torch.int32)
        return [e[0] for e in ev], tab

    @torch.no_grad()
    def sample(self, shape, sampling_kwargs, log_num_per_prog=100, denoise_sample_fn=None, denoise_sample_fn_kwargs=None,
               **kwargs):
        sk = sampling_kwargs
        n = sk["num_timesteps"]
        times, tab = self.plan(n)
        if n > 250:
            warnings.warn("according to the PNDM paper, most gains can be reaped when timestep<250, so it is not "
                          "meaningful to set a timestep larger than 250")
        dev = torch.device(self.device)
        B, Cc = shape[0], shape[1]
        hw = int(np.prod(shape[2:]))
        x_T = kwargs.get("x_T")
        # a private copy: the trajectory is updated in place below / in the captured step
        img = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev, torch.float32, copy=True).contiguous()
        runner = _StepRunner(denoise_sample_fn, denoise_sample_fn_kwargs or {})
        lib = runner.lib
        tab_dev = tab.to(dev)
        # PNDM ignores dtp and noise_dropout: only the model / guidance conditions of the captured step apply
        if _graph_ok(runner, dict(sk, noise_dropout=0, dtp=1), kwargs):
            g = _GraphedPNDMStep.get(runner, img, "pndm", 0)
            ts_dev = torch.tensor(times, dtype=torch.long, device=dev).view(-1, 1).expand(len(times), B).contiguous()
            for k in range(len(times)):
                g.step(ts_dev[k], tab_dev[k])
            img = g.img.clone()                     # the static buffer belongs to the cached graph
            return img, dict(pred_x0=img)
        acc, base = torch.empty_like(img), torch.empty_like(img)
        ring = torch.empty((3,) + tuple(img.shape), device=dev)
        for k, t in enumerate(times):
            ts = torch.full((B,), t, device=dev, dtype=torch.long)
            eps, mode, w, bb, cc = runner.eps(img, ts)
            nxt = torch.empty_like(img)             # a new image per evaluation, as the reference's step returns
            L.check(lib.sgd_pndm_step(_ptr(img), _ptr(eps), mode, w, _ptr(tab_dev[k]), _ptr(acc), _ptr(base), _ptr(ring),
                                      bb, cc, hw, _ptr(nxt), _stream()), "sgd_pndm_step")
            img = nxt
        return img, dict(pred_x0=img)


def to_uint8(x):
    """clip_unnormalize_to_zero_to_255 (diffusion_utils/util.py:99-100)"""
    if x.device.type != "cuda" or x.numel() == 0:
        return ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8)         # snapshots the DDIM path moved to host
    x = x.contiguous().float()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.check(L.load().sgd_to_uint8(_ptr(x), x.numel(), _ptr(out), _stream()), "sgd_to_uint8")
    return out


class LatentDiffusion(nn.Module):
    """diffusion/ddpm.py:24-126 (parameterization eps|x0, loss l1|l2|huber; samplers native, ddim, plms and pndm --
    the reference's 'tero' fails inside its own p_sample_loop)"""

    def __init__(self, **kwargs):
        super().__init__()
        self.hparams = _Obj(kwargs)
        self.sampler = Schedule_DDPM(**kwargs)
        h = self.hparams
        self.sampler_list = {
            "native": self.sampler,
            "ddim": DDIMSampler(ddpm_num_timesteps=h.num_timesteps, device=h.device, sampler_type="ddim"),
            "plms": DDIMSampler(ddpm_num_timesteps=h.num_timesteps, device=h.device, sampler_type="plms"),
            "pndm": PNDM_Sampler(ddpm_num_timesteps=h.num_timesteps, beta_start=h.linear_start, beta_end=h.linear_end,
                                 beta_schedule=h.beta_schedule, device=h.device),
        }

    def set_denoise_fn(self, denoise_fn, denoise_sample_fn):
        self.denoise_fn = denoise_fn

        def _denoise_sample_fn(*args, **kwargs):
            return denoise_sample_fn(*args, **kwargs)

        _denoise_sample_fn._sgdm_inner = denoise_sample_fn
        self.denoise_sample_fn = _denoise_sample_fn

    def forward_tao(self, x, **kwargs):
        return self.forward(x, **kwargs)

    def forward(self, x, *args, **kwargs):
        t = torch.randint(0, self.hparams.num_timesteps, (len(x),), device=x.device).long()
        return self.p_losses(x, t, *args, **kwargs)

    def p_losses(self, x_start, t, noise=None, *args, **kwargs):
        from .train import p_losses_hip
        return p_losses_hip(self, x_start, t, noise, *args, **kwargs)

    @torch.no_grad()
    def p_sample_loop(self, sampling_method, shape, sampling_kwargs, **kwargs):
        sk = copy.deepcopy({k: v for k, v in sampling_kwargs.items()})
        sk.update(dict(alphas_cumprod=self.sampler.alphas_cumprod,
                       alphas_cumprod_prev=self.sampler.alphas_cumprod_prev, betas=self.sampler.betas))
        kwargs.pop("condition_kwargs", None)
        samples, inter = self.sampler_list[sampling_method].sample(
            shape=shape, denoise_sample_fn=self.denoise_sample_fn, sampling_kwargs=sk, **kwargs)
        samples = to_uint8(samples)
        inter["pred_x0"] = to_uint8(inter["pred_x0"])
        # end of a trajectory: the one place this path synchronises anyway -- a conv launch whose balanced tail timed out has
        # poisoned its outputs with NaN and flagged its workspace; raise here instead of handing NaN images on
        unet = _unet_of(getattr(self.denoise_sample_fn, "_sgdm_inner", self.denoise_sample_fn))
        if unet is not None:
            for eng in list(unet._engines.values()):
                eng.check_health()
        return samples, inter

    def vis_schedule(self):
        """ddpm.py:124-126 -> ddpm_sampler.py:240-243: a dict of wandb line plots of the schedule, logged once on the
        first training batch (lightning_module.py:116-122).  The plotting helper is the reference's own
        (diffusion_utils/taokit/wandb_utils.py:44-79, needs wandb); it is used when the checkout is importable, otherwise
        there is nothing to log and the caller's ``logger.experiment.log({})`` is a no-op."""
        return self.sampler.vis_schedule()
