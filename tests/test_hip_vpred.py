"""parameterization='v' on the HIP path (csrc/vpred.hip: sgd_q_sample_v, sgd_v_to_eps; sgdm_amd/diffusion.py:
_StepRunner.v_to_eps; sgdm_amd/train.py: p_losses_hip).  v = sa[t] * noise - s1[t] * x_start with sa = sqrt(alphas_cumprod),
s1 = sqrt(1 - alphas_cumprod) (Salimans & Ho 2022).  The reference has no such parameterization; the expected values are the
formulas restated here -- in torch fp32 in the kernels' documented operation order (bit-exact gates) -- and the project's own
unchanged 'eps' path fed the same function in the other variable (equivalence gates).  GPU only.

Every test prints the figure it asserts on (run with -s).  Measured on the MI355X (bound 1e-5 rel-L2): 'v' fed v_fn against
'eps' fed eps_fn, teacher-forced, worst step: native 1.6e-9, ddim 1.4e-7 / 3.7e-8 (eta 0 / 1), plms 1.6e-7, pndm 6.5e-8,
dpmsolver 7.4e-9; fused-CFG v against the restated method: ddim 6.7e-8, dpmsolver 0.0."""
import pytest
import torch

from conftest import max_rel, rel_l2
from test_hip_unet import build_model

pytestmark = pytest.mark.gpu

B, S = 2, 16
SHAPE = (B, 3, S, S)


@pytest.fixture(scope="module")
def model():
    return build_model("uf_label_c32_s16", "f16x3")[0]


@pytest.fixture(scope="module")
def cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


def _diffusion(par, model=None):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, parameterization=par))
    if model is not None:
        d.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    return d


def _sk(d, method, steps, **kw):
    """sampling kwargs of a direct ``sampler.sample`` call: dynamic_input/misc.py:128-141 plus what p_sample_loop adds"""
    sk = dict(sampling_method=method, vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True,
              dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True,
              disable_tqdm=True, alphas_cumprod=d.sampler.alphas_cumprod, parameterization=d.hparams.parameterization)
    if d.hparams.parameterization == "v":
        sk.update(sqrt_alphas_cumprod=d.sampler.sqrt_alphas_cumprod,
                  sqrt_one_minus_alphas_cumprod=d.sampler.sqrt_one_minus_alphas_cumprod)
    return dict(sk, **kw)


def _tables():
    s = _diffusion("v").sampler
    return s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("t,shape", [([0, 999, 412], (3, 5, 7)), ([999, 0], (3, 16, 16))])
def test_q_sample_v_kernel_is_bit_exact(t, shape):
    """x_noisy carries the bits of sgd_q_sample, v those of sa[t] * noise - s1[t] * x0 in torch fp32 (two rounded products)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    sa, s1 = _tables()
    n = len(t)
    g = torch.Generator().manual_seed(11 + n)
    x0, noise = torch.randn(n, *shape, generator=g), torch.randn(n, *shape, generator=g)
    xd, nd, td = x0.cuda(), noise.cuda(), torch.tensor(t, dtype=torch.long).cuda()
    chw = x0[0].numel()
    ref, xn, v = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    L.check(lib.sgd_q_sample(_ptr(xd), _ptr(nd), _ptr(td), _ptr(sa), _ptr(s1), n, chw, _ptr(ref), _st()), "sgd_q_sample")
    L.check(lib.sgd_q_sample_v(_ptr(xd), _ptr(nd), _ptr(td), _ptr(sa), _ptr(s1), n, chw, _ptr(xn), _ptr(v), _st()),
            "sgd_q_sample_v")
    torch.cuda.synchronize()
    assert torch.equal(xn, ref)
    a, s = sa.cpu()[t].view(n, 1, 1, 1), s1.cpu()[t].view(n, 1, 1, 1)
    assert torch.equal(v.cpu(), a * noise - s * x0)
    assert torch.equal(xn.cpu(), a * x0 + s * noise)


def _guided32(v, mode, w, b):
    """the three un-contracted guided forms in torch fp32 (1 - w / 1 + w formed in fp32, as the kernels do)"""
    vc, vu = v[:b], v[b:]
    wt, one = torch.tensor(w, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32)
    return vc if mode == 0 else (one - wt) * vu + wt * vc if mode == 1 else (one + wt) * vc - wt * vu


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("t,c,hw", [([999, 0], 3, 35), ([17, 999, 0], 4, 256)])
def test_v_to_eps_kernel_is_bit_exact(t, c, hw, mode):
    """guided form first, then sa * v_g + s1 * x, as [b, hw, c]; then the same guided output as b*c one-channel planes
    (the generic denoise_sample_fn path: c = 1, one t per plane)"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    sa, s1 = _tables()
    b, w = len(t), 2.0
    g = torch.Generator().manual_seed(100 * mode + hw)
    x = torch.randn(b, c, hw, generator=g)
    v = torch.randn(2 * b if mode else b, hw, c, generator=g)
    a, s = sa.cpu()[t].view(b, 1, 1), s1.cpu()[t].view(b, 1, 1)
    vg = _guided32(v, mode, w, b)
    want = a * vg + s * x.permute(0, 2, 1)
    xd, vd, td = x.cuda(), v.cuda(), torch.tensor(t, dtype=torch.long).cuda()
    out = torch.full((b, hw, c), float("nan"), device="cuda")
    L.check(lib.sgd_v_to_eps(_ptr(xd), _ptr(vd), _ptr(td), _ptr(sa), _ptr(s1), mode, w, b, c, hw, _ptr(out), _st()),
            "sgd_v_to_eps")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want), float((out.cpu() - want).abs().max())
    # plane form: the guided NCHW output
    gd = vg.permute(0, 2, 1).contiguous().cuda()                    # [b, c, hw]
    tp = td.repeat_interleave(c)
    planes = torch.full((b, c, hw), float("nan"), device="cuda")
    L.check(lib.sgd_v_to_eps(_ptr(xd), _ptr(gd), _ptr(tp), _ptr(sa), _ptr(s1), 0, 0.0, b * c, 1, hw, _ptr(planes), _st()),
            "sgd_v_to_eps")
    torch.cuda.synchronize()
    assert torch.equal(planes.cpu(), want.permute(0, 2, 1))


def test_entry_points_refuse_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    f, t = torch.zeros(64, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    args = dict(x=_ptr(f), v=_ptr(f), t=_ptr(t), sa=_ptr(f), s1=_ptr(f), mode=0, w=0.0, b=1, c=1, hw=8, out=_ptr(f), st=_st())
    call = lambda **k: lib.sgd_v_to_eps(*dict(args, **k).values())          # (keyword order is the C argument order)
    for bad in (dict(x=None), dict(v=None), dict(t=None), dict(sa=None), dict(s1=None), dict(out=None), dict(b=0), dict(c=-1),
                dict(hw=0), dict(mode=3), dict(mode=-1), dict(b=2 ** 30)):
        assert call(**bad) == 1, bad                                         # SGD_ERR_ARG: refused before any launch
    args = dict(x0=_ptr(f), noise=_ptr(f), t=_ptr(t), sa=_ptr(f), s1=_ptr(f), b=1, chw=8, xn=_ptr(f), v=_ptr(f), st=_st())
    call = lambda **k: lib.sgd_q_sample_v(*dict(args, **k).values())
    for bad in (dict(x0=None), dict(noise=None), dict(t=None), dict(sa=None), dict(s1=None), dict(xn=None), dict(v=None),
                dict(b=0), dict(chw=0), dict(b=2 ** 20, chw=2 ** 50)):
        assert call(**bad) == 1, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------- the two parameterizations agree, every sampler

def _extra(method, g):
    """(steps, sampling kwargs, sample() kwargs) of one equivalence case"""
    if method == "native":          # the last 20 steps of the 1000, recorded z
        z = torch.randn(20, *SHAPE, generator=g)
        return 1000, {}, dict(step_indices=list(range(19, -1, -1)), noise_fn=lambda i: z[i])
    if method in ("ddim0", "ddim1"):
        z = torch.randn(10, *SHAPE, generator=g)
        return 10, dict(ddim_eta=float(method[-1])), dict(noise_fn=lambda i: z[i])
    if method == "plms":
        # num_timesteps = 6 gives the 7 table times range(0, 1000, 1000 // 6); one draw per p_sample_plms call, 7 + 1
        z = torch.randn(len(range(0, 1000, 1000 // 6)) + 1, *SHAPE, generator=g)
        return 6, {}, dict(noise_fn=lambda i: z[i])
    return 10, {}, {}


@pytest.mark.parametrize("case", ["native", "ddim0", "ddim1", "plms", "pndm", "dpmsolver"])
def test_v_run_fed_v_fn_lands_on_eps_run_fed_eps_fn(case, model, cond):
    """eps_fn: the HIP UNet's guided output.  v_fn = (eps_fn - s1 x) / sa, formed in float64 and rounded once.  The 'eps' run
    is the project's unchanged path and the yardstick; it records every step input X[k] and output E[k].  The 'v' run is
    teacher-forced: its denoiser overwrites the step input it is handed (the stepper's own image) with X[k] and returns
    v_fn(X[k]); what it was handed -- the result of its previous step from X[k-1] -- and the final image must lie within
    1e-5 rel-L2 of the 'eps' run's (the bound of a sampler update against its float64 restatement)"""
    method = case.rstrip("01")
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    x_T = torch.randn(*SHAPE, generator=g)
    steps, skx, kwx = _extra(case, g)
    X, T, E = [], [], []

    def eps_fn(x, t, **_):
        X.append(x.clone())
        T.append(t.clone())
        E.append(model.forward_with_cond_scale(x, t, cond=cond, layout=None, cond_scale=2.0).clone())
        return E[-1].clone()

    d_e, d_v = _diffusion("eps"), _diffusion("v")
    want, _ = d_e.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d_e, method, steps, **skx), denoise_sample_fn=eps_fn,
                                              denoise_sample_fn_kwargs={}, x_T=x_T, **kwx)
    want = want.clone()
    sa, s1 = (a.double() for a in _tables())
    V = [((e.double() - s1[t].view(B, 1, 1, 1) * x.double()) / sa[t].view(B, 1, 1, 1)).float() for x, t, e in zip(X, T, E)]
    got = []

    def v_fn(x, t, **_):
        k = len(got)
        assert torch.equal(t, T[k]), (k, t, T[k])
        got.append(x.clone())
        x.copy_(X[k])                   # teacher forcing: the step starts from the 'eps' run's input
        return V[k].clone()

    final, _ = d_v.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d_v, method, steps, **skx), denoise_sample_fn=v_fn,
                                               denoise_sample_fn_kwargs={}, x_T=x_T, **kwx)
    assert len(got) == len(X) >= (20 if method == "native" else 7)
    assert torch.equal(got[0], X[0])
    errs = [rel_l2(a, b) for a, b in zip(got[1:], X[1:])] + [rel_l2(final, want)]
    print(f"v vs eps, teacher-forced, {case}: {len(errs)} steps, max rel_l2 {max(errs):.3e} (final {errs[-1]:.3e})")
    assert torch.isfinite(final).all()
    assert max(errs) < 1e-5, errs


# -------------------------------------------------------------- fused-CFG path on the drop-in UNet, its output read as v

def _restate(method, d, x, v, t, row, hist):
    """one step of the method in torch fp32: convert (sa v_g + s1 x at the UNet's time), then the sampler's own update
    with the row of its own table; returns (x_next, x0)"""
    sa, s1 = d.sampler.sqrt_alphas_cumprod[t].view(B, 1, 1, 1), d.sampler.sqrt_one_minus_alphas_cumprod[t].view(B, 1, 1, 1)
    e = sa * v + s1 * x
    if method == "ddim":            # csrc/misc.hip: ddim_step_kernel at eta = 0
        s1m, a_t, a_prev, sigma = (row[j] for j in range(4))
        x0 = ((x - s1m * e) / a_t.sqrt()).clamp(-1, 1)
        return a_prev.sqrt() * x0 + (1.0 - a_prev - sigma * sigma).sqrt() * e, x0
    s1ma, rsa, A, Bc, cc, cp = (row[j] for j in range(6))       # csrc/dpm.hip
    x0 = ((x - s1ma * e) * rsa).clamp(-1, 1)
    D = cc * x0 if float(cp) == 0.0 else cc * x0 + cp * hist
    return A * x + Bc * D, x0


@pytest.mark.parametrize("method", ["ddim", "dpmsolver"])
def test_fused_cfg_v_captured_equals_eager_and_the_restated_method(method, model, cond):
    d = _diffusion("v", model)
    s = d.sampler_list[method]
    dkw = dict(cond=cond, layout=None, cond_scale=2.0)
    x_T = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(41)).cuda()
    if method == "ddim":
        s.make_schedule(_sk(d, method, 10))
        times, tab = [int(v) for v in s.ddim_timesteps], s.step_table
    else:
        ts, tab = s.plan(_sk(d, method, 10))
        times = [int(v) for v in ts]
    n = len(times)
    out = {}
    for graph in (False, True):
        torch.manual_seed(5)
        # (a private x_T per run: the eager DDIM step ping-pongs between the start image's own buffer and a second one)
        final, inter = s.sample(shape=SHAPE, sampling_kwargs=_sk(d, method, 10, hip_graph=graph, log_num_per_prog=n + 1),
                                denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(dkw), x_T=x_T.clone())
        out[graph] = (final.cpu(), inter["x_inter"].cpu(), inter["pred_x0"].cpu())
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    final, x_inter, _ = out[True]
    assert tuple(x_inter.shape) == (n,) + SHAPE and torch.equal(x_inter[-1], final)
    # teacher-forced: the restated method starts every step from the sampler's own step input
    ins = [x_T.cpu()] + list(x_inter[:-1])
    tab, errs, hist = tab.cuda(), [], None
    for k, index in enumerate(reversed(range(n))):
        x = ins[k].cuda()
        t = torch.full((B,), times[index], dtype=torch.long, device="cuda")
        v = model.forward_with_cond_scale(x, t, **dkw)
        nxt, hist = _restate(method, d, x, v, t, tab[index], hist)
        errs.append(rel_l2(x_inter[k], nxt.cpu()))
    print(f"fused-CFG v, {method}: captured == eager; vs restated torch fp32, teacher-forced: max rel_l2 {max(errs):.3e}")
    assert max(errs) < 1e-5, errs
    # read as eps, the same output gives another trajectory
    d_e = _diffusion("eps", model)
    torch.manual_seed(5)
    other, _ = d_e.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d_e, method, 10), denoise_sample_fn=d_e.denoise_sample_fn,
                                               denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)
    assert not torch.equal(other.cpu(), final)


@pytest.mark.parametrize("method", ["ddim", "pndm"])
def test_captured_eps_trajectory_is_untouched_by_a_v_one_on_the_same_model(method, model, cond, monkeypatch):
    """the captured step is cached on the model: 'v' must get a graph of its own"""
    from sgdm_amd import diffusion as Dm
    built = []
    orig = Dm._GraphedStep.__init__

    def init(self, runner, *a, **k):
        built.append(runner.v is not None)
        return orig(self, runner, *a, **k)
    monkeypatch.setattr(Dm._GraphedStep, "__init__", init)
    model.__dict__.pop("_hip_graph_steps", None)
    dkw = dict(cond=cond, layout=None, cond_scale=2.0)
    x_T = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(42)).cuda()
    runs = []
    for par in ("eps", "v", "eps", "v"):
        d = _diffusion(par, model)
        torch.manual_seed(6)
        samples, _ = d.p_sample_loop(method, SHAPE, _sk(d, method, 10, hip_graph=True), denoise_sample_fn_kwargs=dict(dkw),
                                     condition_kwargs={}, x_T=x_T)
        runs.append(samples.cpu())
    assert built == [False, True]                   # one capture each, both reused
    assert torch.equal(runs[0], runs[2]) and torch.equal(runs[1], runs[3])
    assert not torch.equal(runs[0], runs[1])


# --------------------------------------------------------------------------------------------------------------- training

def test_training_step_with_v_target():
    """one p_losses + backward on the c32 model: the loss against the torch restatement on the same x_noisy and model
    output, the gradients against the same step run with the restated target through the existing l2 path (_MSEFn)"""
    from sgdm_amd.synth import synth_batch
    from sgdm_amd.losses import _MSEFn
    m, entry = build_model("uf_clusterlayout_c32_s16", "f32")
    m.train()
    d = _diffusion("v").train()
    seen = {}

    def denoise_fn(x, t, **kw):
        out = m.forward(x, t, **kw)
        seen["x_noisy"], seen["out"] = x.detach().clone(), out[0].detach().clone()
        return out

    d.set_denoise_fn(denoise_fn, m.forward_with_cond_scale)
    kw = entry["ctor"]
    n = 4
    batch = synth_batch(kw["condition_method"], n, S, kw["cond_dim"], entry["layout_dim"], seed=26)
    g = torch.Generator().manual_seed(3)
    x0, noise = batch["image"].cuda(), torch.randn(n, 3, S, S, generator=g).cuda()
    t = torch.tensor([0, 999, 250, 731]).cuda()
    ukw = dict(cond=batch["cond"].float().cuda(), layout=batch["layout"].cuda(), cond_drop_prob=0.5,
               cond_drop_mask=torch.tensor([True, False, False, True]).cuda())
    loss, ld = d.p_losses(x0, t, noise, **ukw)
    loss.backward()
    params = [p for p in m.parameters() if p.requires_grad]
    first, last = params[0].grad.clone(), params[-1].grad.clone()
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(n, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(n, 1, 1, 1)
    assert torch.equal(seen["x_noisy"], sa * x0 + s1 * noise)
    target = sa * noise - s1 * x0
    want = ((target.double() - seen["out"].double()) ** 2).reshape(n, -1).mean(1)
    err_l = abs(float(loss) - float(want.mean())) / float(want.mean())
    assert sorted(ld) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert max_rel(ld["train/epoch_stats_y"].cpu(), want.cpu()) < 1e-6
    # the same step with an explicit target
    m.zero_grad(set_to_none=True)
    out = m.forward(seen["x_noisy"], t, **ukw)[0]
    assert torch.equal(out.detach(), seen["out"])
    _MSEFn.apply(out, target).mean().backward()
    err_f, err_b = max_rel(first, params[0].grad), max_rel(last, params[-1].grad)
    print(f"v training step: loss rel err {err_l:.2e}; grad first / last parameter vs explicit target {err_f:.2e} / {err_b:.2e}")
    assert float(params[0].grad.abs().max()) > 0 and float(params[-1].grad.abs().max()) > 0
    assert err_l < 1e-6
    assert err_f < 1e-4 and err_b < 1e-4
