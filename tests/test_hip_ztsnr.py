"""Zero-terminal-SNR schedules on the HIP path (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are
Flawed"): hparam zero_terminal_snr, sampling kwargs timestep_spacing='trailing' and v_form='data' (csrc/vstep.hip: sgd_v_step;
sgdm_amd/diffusion.py: _VUpdate, v_form_option).  The reference has none of this; the expected values are the formulas
restated here -- torch fp32 in the kernel's documented operation order where the gate is bit-equality, float64 elsewhere -- and
the project's own unchanged eps form of 'v' on the ordinary schedule.  GPU only.

Every test prints the figure it asserts on (run with -s).  The bound 1e-5 rel-L2 is the one tests/test_hip_vpred.py and
tests/test_hip_cfg_schedule.py hold the same kind of comparison to.  Measured on the MI355X, worst step:
zero-terminal-SNR trajectories against float64, teacher-forced: native 5.5e-8, ddim 5.2e-8 / 5.9e-8 (eta 0 / 1), dpmsolver
5.6e-8 (uniform trailing) / 9.2e-8 (logsnr); data form against eps form on the ordinary schedule: native 5.2e-8, ddim 2.3e-7 /
2.9e-7, dpmsolver 2.6e-7; training loss 1.0e-8 relative from the restatement."""
import numpy as np
import pytest
import torch

from conftest import max_rel, rel_l2
from test_hip_unet import build_model
from test_hip_vpred import B, S, SHAPE, _guided32, _sk, _st

pytestmark = pytest.mark.gpu

T, W = 1000, 2.0


@pytest.fixture(scope="module")
def model():
    return build_model("uf_label_c32_s16", "f16x3")[0]


@pytest.fixture(scope="module")
def cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


def _diffusion(model=None, zt=True, par="v"):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    kw = dict(bench.MODEL_PARAMS, parameterization=par)
    if zt:
        kw["zero_terminal_snr"] = True
    d = LatentDiffusion(device="cuda", **kw)
    if model is not None:
        d.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    return d


def _x_T(seed):
    return torch.randn(*SHAPE, generator=torch.Generator().manual_seed(seed)).cuda()


# ----------------------------------------------------------------------------------------------------------------- kernel

def _rows(d):
    """one row of each sampler kind from the zero-terminal-SNR schedule's own tables, the singular ones included, and a
    'dpmsolver' row whose kh is the -0.0 the plan gives the row after the singular one: (name, row [8], has noise)"""
    s = d.sampler
    nat = s.vstep_table([0.9] * T)
    dd = d.sampler_list["ddim"]
    dd.make_schedule(_sk(d, "ddim", 10, ddim_eta=0.5, timestep_spacing="trailing"))
    ddim = dd.vstep_table(0.9)
    _, dpm = d.sampler_list["dpmsolver"].plan(_sk(d, "dpmsolver", 10, dpm_spacing="uniform", timestep_spacing="trailing"), "data")
    rows = [("native T-1", nat[T - 1], True), ("native 412", nat[412], True), ("native 0", nat[0], True),
            ("ddim T-1", ddim[-1], True), ("ddim mid", ddim[4], True), ("dpm T-1", dpm[-1], False),
            ("dpm kh=-0", dpm[-2], False), ("dpm 2nd order", dpm[3], False)]
    assert float(nat[T - 1][0]) == 0.0 and float(nat[0][3]) == 0.0 and float(ddim[4][2]) != 0.0 and float(ddim[4][3]) != 0.0
    assert float(dpm[-2][4]) == 0.0 and float(dpm[-1][4]) == 0.0 and float(dpm[3][4]) != 0.0
    return rows


def _restate32(x, v, z, hist, mode, w, t, sa, s1, row, clip):
    """include/sgdm_hip.h, sgd_v_step, in torch fp32 on the host: every product rounded before it is added, in that order"""
    b = x.shape[0]
    vg = _guided32(v, mode, w, b).permute(0, 2, 1)                          # [b, c, hw]
    a, s = sa[t].view(b, 1, 1), s1[t].view(b, 1, 1)
    x0 = a * x - s * vg
    eps = a * vg + s * x
    if clip:
        x0 = x0.clamp(-1, 1)
    kx, k0, ke, kz, kh = (row[j] for j in range(5))
    acc = kx * x + k0 * x0
    if float(ke) != 0.0:
        acc = acc + ke * eps
    if float(kh) != 0.0:
        acc = acc + kh * hist
    if float(kz) != 0.0:
        acc = acc + kz * z
    return acc, x0, vg.contiguous()


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("ts,c,hw", [([T - 1, 0, 412], 3, 35), ([T - 1, 0], 4, 256), ([412, T - 1], 4, 256)])
def test_v_step_kernel_is_bit_exact(ts, c, hw, mode, clip):
    """[b, hw, c] network output with each cfg_mode, then the same guided output as b*c one-channel planes; in place and out of
    place; rows without history over a NaN-filled history, rows without noise with z = NULL"""
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    d = _diffusion()
    sa_d, s1_d = d.sampler.sqrt_alphas_cumprod, d.sampler.sqrt_one_minus_alphas_cumprod
    sa, s1 = sa_d.cpu(), s1_d.cpu()
    assert float(sa[T - 1]) == 0.0 and float(s1[T - 1]) == 1.0
    b = len(ts)
    g = torch.Generator().manual_seed(1000 * mode + hw + clip)
    x = 1.3 * torch.randn(b, c, hw, generator=g)
    v = 1.3 * torch.randn(2 * b if mode else b, hw, c, generator=g)
    z, hist = torch.randn(b, c, hw, generator=g), torch.randn(b, c, hw, generator=g)
    t = torch.tensor(ts, dtype=torch.long)
    xd, vd, zd, td = x.cuda(), v.cuda(), z.cuda(), t.cuda()
    tp = td.repeat_interleave(c)
    worst = 0.0
    for name, row, noise in _rows(d):
        uses_hist = float(row[4]) != 0.0
        want, want_x0, vg = _restate32(x, v, z, hist, mode, W, t, sa, s1, row, clip)
        assert torch.isfinite(want).all() and torch.isfinite(want_x0).all()
        if clip:
            assert float(want_x0.abs().max()) == 1.0            # the case exercises the clamp
        rd = row.cuda()
        hd = (hist if uses_hist else torch.full_like(hist, float("nan"))).cuda()
        out = torch.full((b, c, hw), float("nan"), device="cuda")
        args = lambda x_in, v_in, m, tt, bb, cc, h, o: (_ptr(x_in), _ptr(v_in), _ptr(zd) if noise else None, m, W if m else 0.0,
                                                        _ptr(tt), _ptr(sa_d), _ptr(s1_d), rd.data_ptr(), _ptr(h), clip, bb, cc, hw,
                                                        _ptr(o), _st())
        L.check(lib.sgd_v_step(*args(xd, vd, mode, td, b, c, hd, out)), "sgd_v_step")
        torch.cuda.synchronize()
        diff = float((out.cpu() - want).abs().max())
        worst = max(worst, diff)
        assert torch.isfinite(out).all() and torch.equal(out.cpu(), want), (name, diff)
        assert torch.equal(hd.cpu(), want_x0), name
        # in place: x_out == x
        xi, hi = xd.clone(), (hist if uses_hist else torch.full_like(hist, float("nan"))).cuda()
        L.check(lib.sgd_v_step(*args(xi, vd, mode, td, b, c, hi, xi)), "sgd_v_step")
        # plane form: the guided NCHW output, c = 1, one t per plane
        gd, hp = vg.cuda(), (hist if uses_hist else torch.full_like(hist, float("nan"))).cuda()
        planes = torch.full((b, c, hw), float("nan"), device="cuda")
        L.check(lib.sgd_v_step(*args(xd, gd, 0, tp, b * c, 1, hp, planes)), "sgd_v_step")
        torch.cuda.synchronize()
        assert torch.equal(xi, out) and torch.equal(hi, hd), name
        assert torch.equal(planes, out) and torch.equal(hp, hd), name
    print(f"sgd_v_step, t {ts}, (b, c, hw) = {(b, c, hw)}, mode {mode}, clip {clip}: 8 rows, max abs diff vs torch fp32 {worst:.1e}")


def test_v_step_refuses_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    lib = L.load()
    f, t = torch.zeros(64, device="cuda"), torch.zeros(2, dtype=torch.long, device="cuda")
    row, h = torch.zeros(8, device="cuda"), torch.zeros(64, device="cuda")
    out = torch.full((8,), -7.0, device="cuda")
    args = dict(x=_ptr(f), v=_ptr(f), z=None, mode=0, w=0.0, t=_ptr(t), sa=_ptr(f), s1=_ptr(f), row=row.data_ptr(), hist=_ptr(h),
                clip=1, b=1, c=1, hw=8, out=_ptr(out), st=_st())
    call = lambda **k: lib.sgd_v_step(*dict(args, **k).values())             # (keyword order is the C argument order)
    for bad in (dict(x=None), dict(v=None), dict(t=None), dict(sa=None), dict(s1=None), dict(row=None), dict(hist=None),
                dict(out=None), dict(b=0), dict(c=-1), dict(hw=0), dict(mode=3), dict(mode=-1), dict(b=2 ** 30),
                dict(b=2 ** 16, c=2 ** 16)):
        assert call(**bad) == 1, bad                                         # SGD_ERR_ARG: refused before any launch
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0                                                       # z = NULL with a row without noise
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ------------------------------------------------------------ trajectories on the zero-terminal-SNR schedule, fused CFG

NATIVE_STEPS = [T - 1] + list(range(19, -1, -1))


def _case(d, case):
    """(method, sampling kwargs, visited (table row, UNet time) in order, sample() kwargs, recorded z per visited step)"""
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    if case == "native":
        z = {i: torch.randn(*SHAPE, generator=g) for i in NATIVE_STEPS}
        sk = _sk(d, "native", T, v_form="data", log_num_per_prog=T + 1)
        return "native", sk, [(i, i) for i in NATIVE_STEPS], dict(step_indices=NATIVE_STEPS, noise_fn=lambda i: z[i]), \
            [z[i] for i in NATIVE_STEPS]
    if case.startswith("ddim"):
        z = torch.randn(10, *SHAPE, generator=g)
        sk = _sk(d, "ddim", 10, v_form="data", ddim_eta=float(case[-1]), timestep_spacing="trailing", log_num_per_prog=11)
        s = d.sampler_list["ddim"]
        s.make_schedule(sk)
        times = [int(v) for v in s.ddim_timesteps]
        return "ddim", sk, [(i, times[i]) for i in reversed(range(10))], dict(noise_fn=lambda i: z[i]), list(z)
    kw = dict(dpm_spacing="uniform", timestep_spacing="trailing") if case == "dpmsolver" else {}       # 'dpmsolver_logsnr'
    sk = _sk(d, "dpmsolver", 10, v_form="data", **kw)
    ts, _ = d.sampler_list["dpmsolver"].plan(sk, "data")
    n = len(ts)
    return "dpmsolver", dict(sk, log_num_per_prog=n + 1), [(i, int(ts[i])) for i in reversed(range(n))], {}, [None] * n


def _run(d, method, sk, cond, x_T, kwx, graph, w=W):
    final, inter = d.sampler_list[method].sample(
        shape=SHAPE, sampling_kwargs=dict(sk, hip_graph=graph), denoise_sample_fn=d.denoise_sample_fn,
        denoise_sample_fn_kwargs=dict(cond=cond, layout=None, cond_scale=w), x_T=x_T.clone(), **kwx)
    return final.cpu(), inter["x_inter"].cpu(), inter["pred_x0"].cpu()


def _method64(d, method, sk, visited):
    """the three methods restated in float64 from the schedule's fp32 buffers, in the variables that are finite at every SNR:
    a closure (k, x, v, z) -> (x_next, x0) over the visited steps; 'dpmsolver' is Lu et al. 2022, Algorithm 2, restated
    from alphas_cumprod alone"""
    s = d.sampler
    sa, s1, ac = s.sqrt_alphas_cumprod.double(), s.sqrt_one_minus_alphas_cumprod.double(), s.alphas_cumprod.double().cpu().numpy()
    times = [t for _, t in visited]

    def x0_eps(k, x, v):
        x0 = sa[times[k]] * x - s1[times[k]] * v
        return (x0.clamp(-1, 1) if sk["clip_denoised"] else x0), sa[times[k]] * v + s1[times[k]] * x

    if method == "native":
        c1, c2, lv = s.posterior_mean_coef1.double(), s.posterior_mean_coef2.double(), s.posterior_log_variance_clipped.double()

        def step(k, x, v, z):
            t = times[k]
            x0, _ = x0_eps(k, x, v)
            return c1[t] * x0 + c2[t] * x + (0.0 if t == 0 else 1.0) * (0.5 * lv[t]).exp() * sk["temperature"] * z, x0
    elif method == "ddim":
        prev = [float(ac[0])] + [float(ac[t]) for t in sorted(times)[:-1]]
        ap = {t: p for t, p in zip(sorted(times), prev)}
        eta = sk["ddim_eta"]

        def step(k, x, v, z):
            t = times[k]
            x0, eps = x0_eps(k, x, v)
            sig = float(eta * np.sqrt((1 - ap[t]) / (1 - ac[t]) * (1 - ac[t] / ap[t])))
            return float(np.sqrt(ap[t])) * x0 + float(np.sqrt(max(1 - ap[t] - sig ** 2, 0.0))) * eps + sig * sk["temperature"] * z, x0
    else:
        with np.errstate(divide="ignore"):
            lam = 0.5 * np.log(ac / (1 - ac))
        prev_t = {t: p for t, p in zip(sorted(times), [0] + sorted(times)[:-1])}
        n = len(times)
        hist = {}

        def step(k, x, v, z):
            t, p = times[k], prev_t[times[k]]
            x0, _ = x0_eps(k, x, v)
            h = lam[p] - lam[t]
            A = float(np.sqrt((1 - ac[p]) / (1 - ac[t])))
            Bq = float(np.sqrt(ac[p]) - A * np.sqrt(ac[t]))
            D = x0
            if k > 0 and not (k == n - 1 and n < 15):                       # second order; lower_order_final below 15 times
                r = float((lam[t] - lam[times[k - 1]]) / h)                       # h_prev / h: 0 after the singular step (h_prev = inf)
                D = x0 if np.isinf(r) else (1 + 1 / (2 * r)) * x0 - 1 / (2 * r) * hist[k - 1]
            hist[k] = x0
            return A * x + Bq * D, x0
    return step


@pytest.mark.parametrize("case", ["native", "ddim0", "ddim1", "dpmsolver", "dpmsolver_logsnr"])
def test_zero_terminal_trajectory_captured_equals_eager_and_the_restated_method(case, model, cond):
    d = _diffusion(model)
    method, sk, visited, kwx, zs = _case(d, case)
    assert visited[0][1] == T - 1 and float(d.sampler.alphas_cumprod[T - 1]) == 0.0
    x_T = _x_T(61)
    out = {}
    for graph in (False, True):
        torch.manual_seed(5)
        out[graph] = _run(d, method, sk, cond, x_T, kwx, graph)
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)
    final, x_inter, pred_x0 = out[True]
    n = len(visited)
    assert tuple(x_inter.shape) == (n,) + SHAPE == tuple(pred_x0.shape) and torch.equal(x_inter[-1], final)
    assert torch.isfinite(x_inter).all() and torch.isfinite(pred_x0).all()
    # teacher-forced: the restated method starts every step from the sampler's own step input
    step = _method64(d, method, sk, visited)
    ins = [x_T.cpu()] + list(x_inter[:-1])
    errs, errs0 = [], []
    for k, (_, t) in enumerate(visited):
        x = ins[k].cuda()
        v = model.forward_with_cond_scale(x, torch.full((B,), t, dtype=torch.long, device="cuda"), cond=cond, layout=None, cond_scale=W)
        nxt, x0 = step(k, x.double(), v.double(), None if zs[k] is None else zs[k].cuda().double())
        errs.append(rel_l2(x_inter[k], nxt.cpu()))
        errs0.append(rel_l2(pred_x0[k], x0.cpu()))
    print(f"zero-terminal-SNR {case}, fused CFG w {W}, data form: {n} steps from t = {visited[0][1]}, captured == eager; vs float64, "
          f"teacher-forced: max rel_l2 {max(errs):.3e} (first step {errs[0]:.3e}), pred_x0 {max(errs0):.3e}")
    assert max(errs) <= 1e-5, errs
    assert max(errs0) <= 1e-5, errs0


def test_zero_terminal_scheduled_guidance_replays_by_the_table(model, cond):
    """cfg_rescale and an interval on the data form: both graphs of the step, counted as the host table says"""
    from sgdm_amd.diffusion import cfg_schedule
    d = _diffusion(model)
    method, sk, visited, kwx, _ = _case(d, "ddim1")
    times = sorted(t for _, t in visited)
    iv = (times[3], times[6])
    flags, _ = cfg_schedule(times, W, model._scale_mode(), iv)
    assert sum(flags) == 4
    sk = dict(sk, cfg_rescale=0.7, cfg_interval=iv)
    model.__dict__.pop("_hip_graph_steps", None)
    x_T, out = _x_T(62), {}
    for graph in (False, True):
        torch.manual_seed(8)
        out[graph] = _run(d, method, sk, cond, x_T, kwx, graph)
    (step,) = model.__dict__["_hip_graph_steps"].values()
    print(f"zero-terminal-SNR ddim-10, rescale 0.7, interval {iv}: replays {step.replays}; captured vs eager max abs diff "
          f"{max(float((a - b).abs().max()) for a, b in zip(out[False], out[True])):.1e}")
    for a, b in zip(out[False], out[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert step.replays == dict(guided=4, cond=6) and step.graph1 is not None and step.upd.kind == "v_ddim"
    torch.manual_seed(8)
    assert not torch.equal(_run(d, method, {k: v for k, v in sk.items() if not k.startswith("cfg_")}, cond, x_T, kwx, True)[0],
                           out[True][0])


def test_p_sample_loop_on_a_zero_terminal_model(model, cond):
    """the public entry: the data form is chosen for the model, the trailing spacing is the caller's"""
    d = _diffusion(model)
    base = {k: v for k, v in _sk(d, "ddim", 10).items() if k not in ("alphas_cumprod", "parameterization")}
    x_T = _x_T(63)
    dkw = dict(cond=cond, layout=None, cond_scale=W)
    for method, kw in (("ddim", dict(timestep_spacing="trailing")), ("dpmsolver", {}), ("plms", dict(num_timesteps=6))):
        torch.manual_seed(3)
        u8, inter = d.p_sample_loop(method, SHAPE, dict(base, **kw), denoise_sample_fn_kwargs=dict(dkw), condition_kwargs={}, x_T=x_T)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == SHAPE and inter["pred_x0"].dtype == torch.uint8
        assert len(set(u8.flatten().tolist())) > 16, method           # an image, not a NaN cast
    with pytest.raises(ValueError, match="alphas_cumprod is 0"):
        d.p_sample_loop("ddim", SHAPE, dict(base, timestep_spacing="trailing", v_form="eps"), denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)


# ------------------------------------------------------------------------------- the two forms agree on the ordinary schedule

def _extra(case, g):
    if case == "native":            # T-1, where the eps form multiplies by 1 / sa = 37, and the last 20 steps
        z = {i: torch.randn(*SHAPE, generator=g) for i in NATIVE_STEPS}
        return "native", T, {}, dict(step_indices=NATIVE_STEPS, noise_fn=lambda i: z[i])
    if case.startswith("ddim"):
        z = torch.randn(10, *SHAPE, generator=g)
        return "ddim", 10, dict(ddim_eta=float(case[-1])), dict(noise_fn=lambda i: z[i])
    return "dpmsolver", 10, {}, {}                                 # 'logsnr' spacing: starts at T-1


@pytest.mark.parametrize("case", ["native", "ddim0", "ddim1", "dpmsolver"])
def test_data_form_lands_on_the_eps_form_on_the_ordinary_schedule(case, model, cond):
    """the same denoiser -- the HIP UNet's guided output read as v -- on the generic (one-channel plane) path.  The 'eps' form
    is the project's unchanged path; it records every step input X[k] and the output V[k].  The 'data' run is teacher-forced
    like tests/test_hip_vpred.py: its denoiser overwrites the step input it is handed with X[k] and returns V[k]; what it was
    handed -- the result of its previous step from X[k-1] -- and the final image are held to 1e-5 rel-L2 of the eps form's"""
    g = torch.Generator().manual_seed(sum(map(ord, case)) + 1)
    x_T = torch.randn(*SHAPE, generator=g)
    method, steps, skx, kwx = _extra(case, g)
    d = _diffusion(zt=False)
    X, Ts, V = [], [], []

    def fn(x, t, **_):
        X.append(x.clone())
        Ts.append(t.clone())
        V.append(model.forward_with_cond_scale(x, t, cond=cond, layout=None, cond_scale=W).clone())
        return V[-1].clone()

    want, _ = d.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d, method, steps, **skx), denoise_sample_fn=fn,
                                            denoise_sample_fn_kwargs={}, x_T=x_T, **kwx)
    want = want.clone()
    got = []

    def forced(x, t, **_):
        k = len(got)
        assert torch.equal(t, Ts[k]), (k, t, Ts[k])
        got.append(x.clone())
        x.copy_(X[k])
        return V[k].clone()

    final, _ = d.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d, method, steps, v_form="data", **skx),
                                             denoise_sample_fn=forced, denoise_sample_fn_kwargs={}, x_T=x_T, **kwx)
    assert len(got) == len(X) >= 7 and torch.equal(got[0], X[0])
    errs = [rel_l2(a, b) for a, b in zip(got[1:], X[1:])] + [rel_l2(final, want)]
    worst = max(range(len(errs)), key=errs.__getitem__)
    print(f"data form vs eps form, ordinary schedule, teacher-forced, {case}: {len(errs)} steps, max rel_l2 {max(errs):.3e} at the "
          f"step from t = {int(Ts[worst][0])} (first step, from t = {int(Ts[0][0])}: {errs[0]:.3e}; final {errs[-1]:.3e})")
    assert torch.isfinite(final).all()
    assert max(errs) <= 1e-5, errs


def test_default_captured_v_trajectory_is_untouched_by_data_form_ones(model, cond, monkeypatch):
    """the captured step is cached on the model: the data form must get entries of its own, and leave the eps form's alone"""
    from sgdm_amd import diffusion as Dm
    built = []
    orig = Dm._GraphedStep.__init__

    def init(self, runner, eng, img, upd):
        built.append((upd.kind, runner.form))
        return orig(self, runner, eng, img, upd)
    monkeypatch.setattr(Dm._GraphedStep, "__init__", init)
    model.__dict__.pop("_hip_graph_steps", None)
    plain, zt = _diffusion(model, zt=False), _diffusion(model)
    dkw = dict(cond=cond, layout=None, cond_scale=W)
    x_T = _x_T(64)

    def run(d, method, **kw):
        torch.manual_seed(6)
        u8, _ = d.p_sample_loop(method, SHAPE, dict(_sk(d, method, 10, hip_graph=True), **kw), denoise_sample_fn_kwargs=dict(dkw),
                                condition_kwargs={}, x_T=x_T)
        return u8.cpu()

    before = run(plain, "ddim")
    data = run(plain, "ddim", v_form="data")
    run(plain, "dpmsolver", v_form="data")
    run(zt, "ddim", timestep_spacing="trailing")
    run(zt, "dpmsolver")
    after = run(plain, "ddim")
    again = run(plain, "ddim", v_form="data")
    print(f"captured steps built: {built}; default ddim 'v' before / after: max abs diff "
          f"{int((before.int() - after.int()).abs().max())}; data form vs eps form, uint8: {int((before.int() - data.int()).abs().max())}")
    assert built == [("ddim", "eps"), ("v_ddim", "data"), ("v_dpmsolver", "data")]      # one capture per kind, each reused
    assert torch.equal(before, after) and torch.equal(data, again)
    assert int((before.int() - data.int()).abs().max()) <= 1                # the two forms are one trajectory up to rounding


# --------------------------------------------------------------------------------------------------------------- training

def test_training_step_at_zero_snr():
    """one p_losses + backward with t = [T-1, 0] on the zero-terminal-SNR schedule: at T-1 x_noisy is the noise and the
    target -x_start; the loss against the torch restatement on the same x_noisy and model output"""
    from sgdm_amd.synth import synth_batch
    m, entry = build_model("uf_clusterlayout_c32_s16", "f32")
    m.train()
    d = _diffusion().train()
    seen = {}

    def denoise_fn(x, t, **kw):
        out = m.forward(x, t, **kw)
        seen["x_noisy"], seen["out"] = x.detach().clone(), out[0].detach().clone()
        return out

    d.set_denoise_fn(denoise_fn, m.forward_with_cond_scale)
    kw = entry["ctor"]
    n = 2
    batch = synth_batch(kw["condition_method"], n, S, kw["cond_dim"], entry["layout_dim"], seed=26)
    x0, noise = batch["image"].cuda(), torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(3)).cuda()
    t = torch.tensor([T - 1, 0]).cuda()
    loss, ld = d.p_losses(x0, t, noise, cond=batch["cond"].float().cuda(), layout=batch["layout"].cuda(), cond_drop_prob=0.5,
                          cond_drop_mask=torch.tensor([True, False]).cuda())
    loss.backward()
    s = d.sampler
    sa, s1 = s.sqrt_alphas_cumprod[t].view(n, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod[t].view(n, 1, 1, 1)
    assert torch.equal(seen["x_noisy"], sa * x0 + s1 * noise) and torch.equal(seen["x_noisy"][0], noise[0])
    target = sa * noise - s1 * x0
    assert torch.equal(target[0], -x0[0])
    want = ((target.double() - seen["out"].double()) ** 2).reshape(n, -1).mean(1)
    err_l = abs(float(loss) - float(want.mean())) / float(want.mean())
    grads = [p.grad for p in m.parameters() if p.requires_grad]
    print(f"zero-terminal-SNR training step, t = [T-1, 0]: loss {float(loss):.6f}, rel err vs restated {err_l:.2e}; "
          f"{len(grads)} gradients, max |g| {max(float(g.abs().max()) for g in grads):.3e}")
    assert np.isfinite(float(loss)) and err_l < 1e-6
    assert max_rel(ld["train/epoch_stats_y"].cpu(), want.cpu()) < 1e-6
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert float(grads[0].abs().max()) > 0 and float(grads[-1].abs().max()) > 0
