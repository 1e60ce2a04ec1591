"""Guidance schedule on the HIP path: limited-interval guidance (Kynkaanniemi et al. 2024; sampling kwarg cfg_interval) and CFG
rescale (Lin et al. 2023, section 3.4; cfg_rescale).  csrc/guide.hip: sgd_cfg_guide; sgdm_amd/diffusion.py: cfg_schedule,
_StepRunner.guide / .eps, _GraphedStep (a pair of graphs when an interval is requested).  The reference has neither; the expected
values are the formulas restated here -- torch fp32 in the kernel's operation order where the gate is bit-equality, float64
elsewhere -- and the project's own unchanged paths at the two degenerate ends.  GPU only.

Every test prints the figure it asserts on (run with -s).  The bound 1e-5 rel-L2 is the one the sampler kernels are held to
against their float64 restatements."""
import itertools

import pytest
import torch

from conftest import rel_l2
from test_hip_unet import build_model
from test_hip_vpred import B, S, SHAPE, _diffusion, _guided32, _sk, _st

pytestmark = pytest.mark.gpu

W, PHI = 2.0, 0.7


@pytest.fixture(scope="module")
def model():
    return build_model("uf_label_c32_s16", "f16x3")[0]


@pytest.fixture(scope="module")
def cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


# ---------------------------------------------------------------------------------------------------------------- kernel

def _guide(out, mode, w, phi, b, c, hw, sentinel=float("nan")):
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    od, wd = out.cuda(), torch.tensor([w], dtype=torch.float32, device="cuda")
    g = torch.full((b, hw, c), sentinel, device="cuda")
    L.check(L.load().sgd_cfg_guide(_ptr(od), mode, _ptr(wd), phi, b, c, hw, _ptr(g), _st()), "sgd_cfg_guide")
    torch.cuda.synchronize()
    return g.cpu()


def _halves(b, c, hw, seed):
    """[2b, hw, c]: halves of different mean and spread, so that the rescale factor is far from 1"""
    g = torch.Generator().manual_seed(seed)
    oc = 0.3 + 1.1 * torch.randn(b, hw, c, generator=g)
    ou = -0.2 + 0.8 * torch.randn(b, hw, c, generator=g)
    return torch.cat((oc, ou), 0)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("b,c,hw", [(3, 3, 35), (2, 4, 256), (1, 3, 16)])
def test_guide_kernel_without_rescale_is_bit_exact(b, c, hw, mode):
    """the two un-contracted guided forms, the weight read from a device float"""
    out = _halves(b, c, hw, 7 * hw + mode)
    for w in (W, 7.5, -0.3):
        got, want = _guide(out, mode, w, 0.0, b, c, hw), _guided32(out, mode, w, b)
        print(f"guide, rescale 0, mode {mode}, (b, c, hw) = {(b, c, hw)}, w = {w}: max abs diff {float((got - want).abs().max()):.1e}")
        assert torch.equal(got, want)


def _rescaled64(out, mode, w, phi, b):
    """float64: guided form, unbiased std per sample, k = phi * s_pos / s_g + (1 - phi); returns (k [b], k * g)"""
    o = out.double()
    oc, ou = o[:b], o[b:]
    g = (1.0 - w) * ou + w * oc if mode == 1 else (1.0 + w) * oc - w * ou
    if oc[0].numel() > 1:
        s_pos, s_g = oc.reshape(b, -1).std(1), g.reshape(b, -1).std(1)
        f = torch.where(s_g > 0, s_pos / s_g.clamp_min(1e-300), torch.ones_like(s_g))
    else:
        f = torch.ones(b, dtype=torch.float64)
    k = phi * f + (1.0 - phi)
    return k, k.view(b, 1, 1) * g


@pytest.mark.parametrize("phi", [0.7, 1.0])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("b,c,hw", [(3, 3, 35), (2, 4, 256), (1, 3, 16), (2, 3, 4096)])
def test_guide_kernel_rescale_against_float64(b, c, hw, mode, phi):
    out = _halves(b, c, hw, 13 * hw + mode)
    got = _guide(out, mode, W, phi, b, c, hw)
    k64, want = _rescaled64(out, mode, W, phi, b)
    # the kernel's factor: out = fl(k * g32) with g32 the bit-exact guided form, so <out, g32> / <g32, g32> is k to ~1e-7
    g32 = _guided32(out, mode, W, b).double().reshape(b, -1)
    k = (got.double().reshape(b, -1) * g32).sum(1) / (g32 * g32).sum(1)
    err, err_k = rel_l2(got, want), float(((k - k64).abs() / k64.abs()).max())
    print(f"guide, rescale {phi}, mode {mode}, (b, c, hw) = {(b, c, hw)}: rel_l2 {err:.2e}, factor k {k64.tolist()} rel err {err_k:.2e}")
    assert float((k64 - 1).abs().min()) > 0.05              # the case exercises the rescale
    assert err <= 1e-5 and err_k <= 1e-5
    if phi == 1.0:                                          # the guided sample takes the conditional sample's std
        s_out, s_pos = got.double().reshape(b, -1).std(1), out[:b].double().reshape(b, -1).std(1)
        err_s = float(((s_out - s_pos).abs() / s_pos).max())
        print(f"    std of the output vs std of the conditional half: rel err {err_s:.2e}")
        assert err_s <= 1e-5
    assert torch.equal(_guide(out, mode, W, phi, b, c, hw), got)            # fixed reduction order: run-to-run identical


def test_guide_kernel_degenerate_samples_and_bad_arguments():
    from sgdm_amd import _lib as L
    from sgdm_amd.unet import _ptr
    # constant halves: s_g = 0 -> f = 1, k = 1 (values whose sums are exact in fp32, so both centred sums are exactly 0)
    for (b, c, hw), mode in itertools.product([(2, 3, 35), (2, 3, 4096)], (1, 2)):
        out = torch.cat((torch.full((b, hw, c), 0.5), torch.full((b, hw, c), -0.25)), 0)
        got, want = _guide(out, mode, W, 0.7, b, c, hw), _guided32(out, mode, W, b)
        print(f"guide, constant halves, mode {mode}, {(b, c, hw)}: output {float(got.flatten()[0])} (guided form {float(want.flatten()[0])})")
        assert torch.isfinite(got).all() and torch.equal(got, want)
    # a one-element sample: f = 1
    out = torch.tensor([1.5, -0.5]).view(2, 1, 1)
    assert torch.equal(_guide(out, 2, W, 1.0, 1, 1, 1), _guided32(out, 2, W, 1))
    # refused before any launch: the output keeps its sentinel
    lib = L.load()
    f, w = torch.ones(2 * 64, device="cuda"), torch.full((1,), 2.0, device="cuda")
    g = torch.full((64,), -7.0, device="cuda")
    args = dict(out=_ptr(f), mode=1, w=_ptr(w), phi=0.5, b=1, c=4, hw=16, g=_ptr(g), st=_st())
    call = lambda **k: lib.sgd_cfg_guide(*dict(args, **k).values())          # (keyword order is the C argument order)
    for bad in (dict(out=None), dict(w=None), dict(g=None), dict(mode=0), dict(mode=3), dict(mode=-1), dict(phi=-0.01),
                dict(phi=1.01), dict(phi=float("nan")), dict(b=0), dict(c=0), dict(hw=-1), dict(b=2 ** 30, c=2, hw=2),
                dict(c=2 ** 20, hw=2 ** 20)):
        assert call(**bad) == 1, bad                                         # SGD_ERR_ARG
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((g != -7.0).all())


# ------------------------------------------------------------------------------------------------------------ trajectories

def _plan(d, method, steps=10):
    """(UNet time per evaluation in table order, coefficient table) of the sampler's own schedule"""
    s = d.sampler_list[method]
    if method == "ddim":
        s.make_schedule(_sk(d, method, steps))
        return [int(v) for v in s.ddim_timesteps], s.step_table
    if method == "pndm":
        return s.plan(steps)
    ts, tab = s.plan(_sk(d, method, steps))
    return [int(v) for v in ts], tab


def _middle(times):
    """an interval that covers the middle evaluations only: the 4th .. 7th smallest of the distinct times"""
    u = sorted(set(times))
    assert len(u) >= 9
    return (u[3], u[6])


def _sample(d, method, cond, x_T, w=W, steps=10, **skx):
    n = len(_plan(d, method, steps)[0])
    final, inter = d.sampler_list[method].sample(
        shape=SHAPE, sampling_kwargs=_sk(d, method, steps, **dict(dict(log_num_per_prog=n + 1), **skx)),
        denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(cond=cond, layout=None, cond_scale=w), x_T=x_T.clone())
    return final.cpu(), inter.get("x_inter", final).cpu()


def _steps(model):
    return list(model.__dict__.get("_hip_graph_steps", {}).values())


def _x_T(seed):
    return torch.randn(*SHAPE, generator=torch.Generator().manual_seed(seed)).cuda()


def _update(method, x, e, row, hist):
    """the sampler's own update in torch fp32 with the row of its own table (csrc/misc.hip: ddim_step_kernel at eta = 0;
    csrc/dpm.hip); returns (x_next, x0)"""
    if method == "ddim":
        s1m, a_t, a_prev, sigma = (row[j] for j in range(4))
        x0 = ((x - s1m * e) / a_t.sqrt()).clamp(-1, 1)
        return a_prev.sqrt() * x0 + (1.0 - a_prev - sigma * sigma).sqrt() * e, x0
    s1ma, rsa, A, Bc, cc, cp = (row[j] for j in range(6))
    x0 = ((x - s1ma * e) * rsa).clamp(-1, 1)
    D = cc * x0 if float(cp) == 0.0 else cc * x0 + cp * hist
    return A * x + Bc * D, x0


@pytest.mark.parametrize("method", ["ddim", "dpmsolver"])
def test_scheduled_trajectory_against_the_restated_method(method, model, cond):
    """teacher-forced: every step of the restatement starts from the sampler's own step input.  Guided evaluations:
    forward_with_cond_scale, rescaled in float64 with the conditional output of forward(cond_drop_prob=0); the others:
    forward(cond_drop_prob=0) alone; then the update restated in torch fp32"""
    d = _diffusion("eps", model)
    times, tab = _plan(d, method)
    iv = _middle(times)
    x_T = _x_T(51)
    torch.manual_seed(7)
    final, x_inter = _sample(d, method, cond, x_T, cfg_rescale=PHI, cfg_interval=iv)
    n = len(times)
    assert tuple(x_inter.shape) == (n,) + SHAPE and torch.equal(x_inter[-1], final)
    ins = [x_T.cpu()] + list(x_inter[:-1])
    tab, errs, hist, guided = tab.cuda(), [], None, 0
    for k, index in enumerate(reversed(range(n))):
        x = ins[k].cuda()
        t = torch.full((B,), times[index], dtype=torch.long, device="cuda")
        oc = model.forward(x, t, cond=cond, layout=None, cond_drop_prob=0.0)[0]
        if iv[0] <= times[index] <= iv[1]:
            g = model.forward_with_cond_scale(x, t, cond=cond, layout=None, cond_scale=W).double()
            s_pos, s_g = oc.double().reshape(B, -1).std(1), g.reshape(B, -1).std(1)
            e = ((PHI * s_pos / s_g + (1.0 - PHI)).view(B, 1, 1, 1) * g).float()
            guided += 1
        else:
            e = oc
        nxt, hist = _update(method, x, e, tab[index], hist)
        errs.append(rel_l2(x_inter[k], nxt.cpu()))
    assert guided == 4
    print(f"scheduled {method}-10 (w {W}, rescale {PHI}, interval {iv}: {guided} of {n} guided) vs restated, teacher-forced: "
          f"max rel_l2 {max(errs):.3e} (final {errs[-1]:.3e})")
    assert torch.isfinite(final).all()
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("par", ["eps", "v"])
@pytest.mark.parametrize("method", ["ddim", "pndm"])
def test_scheduled_captured_equals_eager(method, par, model, cond):
    from sgdm_amd import _lib as L
    from sgdm_amd.diffusion import cfg_schedule
    d = _diffusion(par, model)
    times, _ = _plan(d, method)
    iv = _middle(times)
    flags, _ = cfg_schedule(times, W, model._scale_mode(), iv)
    assert 0 < sum(flags) < len(flags)
    model.__dict__.pop("_hip_graph_steps", None)
    x_T, out = _x_T(52), {}
    for graph in (False, True):
        torch.manual_seed(8)
        out[graph] = _sample(d, method, cond, x_T, cfg_rescale=PHI, cfg_interval=iv, hip_graph=graph)
    diff = max(float((a - b).abs().max()) for a, b in zip(out[False], out[True]))
    (step,) = _steps(model)
    print(f"scheduled {method}/{par}: captured vs eager max abs diff {diff:.1e}; replays {step.replays}, table {sum(flags)} guided of {len(flags)}")
    for a, b in zip(out[False], out[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert step.replays == dict(guided=sum(flags), cond=len(flags) - sum(flags))
    assert step.graph1 is not None and step.eng1 is model._engines[(B, S, S, L.PREC_BY_NAME[model.hip_precision])]
    # guidance in the interval only is another trajectory than guidance throughout
    torch.manual_seed(8)
    assert not torch.equal(_sample(d, method, cond, x_T)[0], out[True][0])


def test_interval_that_hits_nothing_is_the_conditional_trajectory(model, cond):
    """same seed, eta = 1 (the noise matters): today's cond_scale = 1 run of this imagen-type model takes the model's single
    evaluation, forward(cond_drop_prob=p0), on the eager generic path"""
    d = _diffusion("eps", model)
    x_T = _x_T(53)
    torch.manual_seed(9)
    want, _ = _sample(d, "ddim", cond, x_T, w=1.0, ddim_eta=1.0)
    model.__dict__.pop("_hip_graph_steps", None)
    for graph in (True, False):
        torch.manual_seed(9)
        got, _ = _sample(d, "ddim", cond, x_T, cfg_interval=(2, 100), ddim_eta=1.0, hip_graph=graph)
        err = rel_l2(got, want)
        print(f"empty interval ({'captured' if graph else 'eager'}) vs cond_scale=1: rel_l2 {err:.2e}, max abs diff "
              f"{float((got - want).abs().max()):.1e}")
        assert err <= 1e-5
    (step,) = _steps(model)
    assert step.replays == dict(guided=0, cond=10)


def _run_other(d, method, cond, x_T, w=W, **skx):
    """the two samplers the tests above leave out: 'native' (its last 20 steps) and 'plms' (6 -> 7 times, 8 evaluations)"""
    kw = dict(denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(cond=cond, layout=None, cond_scale=w),
              x_T=x_T.clone())
    if method == "native":
        return d.sampler.sample(SHAPE, sampling_kwargs=_sk(d, method, 1000, **skx), step_indices=list(range(19, -1, -1)), **kw)[0].cpu()
    return d.sampler_list[method].sample(shape=SHAPE, sampling_kwargs=_sk(d, method, 6, **skx), **kw)[0].cpu()


@pytest.mark.parametrize("method", ["native", "plms"])
def test_native_and_plms_honour_the_schedule(method, model, cond):
    """an interval that hits nothing is the cond_scale = 1 run under the same seed (noise drawn per step in both samplers);
    an interval that hits some evaluations is a third trajectory, the same captured and eager, with the table's counts"""
    from sgdm_amd import diffusion as Dm
    d = _diffusion("eps", model)
    x_T = _x_T(56)
    # native visits t = 19 .. 0; plms evaluates at 1, 167, .., 997 (and twice on its first step)
    some, none = ((5, 12), (20, 999)) if method == "native" else ((167, 499), (2, 100))
    counts = dict(guided=8, cond=12) if method == "native" else dict(guided=3, cond=5)
    torch.manual_seed(12)
    want = _run_other(d, method, cond, x_T, w=1.0)
    torch.manual_seed(12)
    full = _run_other(d, method, cond, x_T)
    model.__dict__.pop("_hip_graph_steps", None)
    seen = []
    for graph in (True, False):
        torch.manual_seed(12)
        got = _run_other(d, method, cond, x_T, cfg_interval=none, hip_graph=graph)
        err = rel_l2(got, want)
        print(f"{method}, empty interval ({'captured' if graph else 'eager'}) vs cond_scale=1: rel_l2 {err:.2e}, max abs diff "
              f"{float((got - want).abs().max()):.1e}")
        assert err <= 1e-5
        torch.manual_seed(12)
        seen.append(_run_other(d, method, cond, x_T, cfg_interval=some, cfg_rescale=PHI, hip_graph=graph))
    assert torch.isfinite(seen[0]).all() and torch.equal(seen[0], seen[1])
    assert not torch.equal(seen[0], want) and not torch.equal(seen[0], full)
    if method == "native":                              # (plms has no captured step: its eps is the caller's)
        steps = _steps(model)
        assert len(steps) == 2 and steps[1].replays == counts, [s.replays for s in steps]
    else:
        assert not _steps(model)
        flags = Dm.cfg_schedule([997, 831] + list(range(831, 0, -166)), W, 1, some)[0]        # the evaluations' times, in order
        assert dict(guided=sum(flags), cond=len(flags) - sum(flags)) == counts


@pytest.mark.parametrize("method", ["ddim", "dpmsolver"])
def test_full_interval_without_rescale_is_the_fused_path(method, model, cond, monkeypatch):
    """teacher-forced: the scheduled run starts every step from the step input of today's fused run"""
    from sgdm_amd import diffusion as Dm
    d = _diffusion("eps", model)
    x_T = _x_T(54)
    torch.manual_seed(10)
    _, want = _sample(d, method, cond, x_T)
    ins = [x_T] + [x.cuda() for x in want[:-1]]
    orig, k = Dm._GraphedStep.step, itertools.count()

    def step(self, i, *a, **kw):
        self.img.copy_(ins[next(k)])
        return orig(self, i, *a, **kw)
    monkeypatch.setattr(Dm._GraphedStep, "step", step)
    torch.manual_seed(10)
    _, got = _sample(d, method, cond, x_T, cfg_interval=(0, 999))
    assert next(k) == len(ins) == 10
    errs = [rel_l2(a, b) for a, b in zip(got, want)]
    print(f"full interval, rescale 0, {method}-10 vs the fused path, teacher-forced: max rel_l2 {max(errs):.3e}; "
          f"bit-equal: {torch.equal(got, want)}")
    assert max(errs) <= 1e-5, errs


def test_no_residue_and_one_capture_for_a_sweep(model, cond):
    d = _diffusion("eps", model)
    x_T = _x_T(55)
    model.__dict__.pop("_hip_graph_steps", None)
    torch.manual_seed(11)
    before = _sample(d, "ddim", cond, x_T)
    torch.manual_seed(11)
    first = _sample(d, "ddim", cond, x_T, cfg_rescale=PHI, cfg_interval=(301, 601))
    steps = _steps(model)
    assert len(steps) == 2
    torch.manual_seed(11)
    second = _sample(d, "ddim", cond, x_T, w=3.5, cfg_rescale=PHI, cfg_interval=(101, 801))
    assert [id(s) for s in _steps(model)] == [id(s) for s in steps]         # weight and bounds are data: the same step object
    assert steps[1].replays == dict(guided=8, cond=2)
    assert not torch.equal(first[0], second[0])
    torch.manual_seed(11)
    again = _sample(d, "ddim", cond, x_T, cfg_rescale=PHI, cfg_interval=(301, 601))
    torch.manual_seed(11)
    after = _sample(d, "ddim", cond, x_T)
    print(f"default ddim before / after scheduled runs: max abs diff {float((before[1] - after[1]).abs().max()):.1e}; "
          f"scheduled run repeated after a sweep: {float((first[1] - again[1]).abs().max()):.1e}; captured steps {len(_steps(model))}")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert [id(s) for s in _steps(model)] == [id(s) for s in steps]
