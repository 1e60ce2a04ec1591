"""sampling_method='pndm' (sgdm_amd/diffusion.py: PNDM_Sampler, csrc/pndm.hip: sgd_pndm_step) through
LatentDiffusion.p_sample_loop against the reference's own PNDM trajectories (tests/golden/pndm.npz, make_golden_pndm.py).
GPU only."""
import numpy as np
import pytest
import torch

from conftest import load_npz, rel_l2
from test_hip_unet import build_model

pytestmark = pytest.mark.gpu

B, S = 2, 16


def _diffusion(model=None, fn=None):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
    if model is not None:
        d.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    else:
        d.set_denoise_fn(None, fn)
    return d


def _skw(steps, **kw):
    # dynamic_input/misc.py:128-141
    return dict(dict(sampling_method="pndm", vis=None, num_timesteps=steps, ddim_eta=0.0, log_num_per_prog=10,
                     clip_denoised=True, dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False,
                     return_inter_dict=True, disable_tqdm=True), **kw)


def _cond():
    from sgdm_amd.synth import synth_batch
    return synth_batch("label", B, S, 10, seed=23)["cond"].cuda()


def _dkw():
    return dict(cond=_cond(), layout=None, cond_scale=2.0)


@pytest.mark.parametrize("n,calls", [(10, 19), (13, 23)])
def test_teacher_forced_update_is_bit_exact(n, calls):
    """the strict gate: a plain-Python denoiser (generic path, cfg_mode 0) returns the reference's recorded residual for
    each call; the kernel's update -- no contraction, the reference's fp32 op order, host scalars from the reference's
    torch expressions -- must then reproduce every UNet input and the final fp32 image with max abs diff 0"""
    v = load_npz("pndm.npz")
    tag = f"pndm{n}"
    t_ref, x_in, eps = v[tag + ".t"], torch.from_numpy(v[tag + ".x_in"]), torch.from_numpy(v[tag + ".eps"])
    seen = []

    def fn(x, t, **_):
        k = len(seen)
        assert torch.equal(t.cpu(), torch.full((B,), int(t_ref[k]), dtype=torch.long)), (k, t)
        seen.append(x.detach().cpu().clone())
        return eps[k].cuda()

    d = _diffusion(fn=fn)
    x_T = torch.from_numpy(v[tag + ".x_T"])
    final, inter = d.sampler_list["pndm"].sample(shape=(B, 3, S, S), sampling_kwargs=_skw(n), denoise_sample_fn=d.denoise_sample_fn,
                                                 denoise_sample_fn_kwargs={}, x_T=x_T)
    assert len(seen) == calls
    diff_in = max(float((a - x_in[k]).abs().max()) for k, a in enumerate(seen))
    diff_out = float((final.cpu() - torch.from_numpy(v[tag + ".final"])).abs().max())
    print(f"pndm{n} teacher-forced: max abs diff inputs {diff_in}, final {diff_out}")
    assert diff_in == 0.0 and diff_out == 0.0
    assert set(inter) == {"pred_x0"}
    seen.clear()
    samples, inter = d.p_sample_loop("pndm", (B, 3, S, S), _skw(n), denoise_sample_fn_kwargs={}, condition_kwargs={}, x_T=x_T)
    assert len(seen) == calls
    assert torch.equal(samples.cpu(), torch.from_numpy(v[tag + ".samples_u8"]))


def test_free_running_vs_reference():
    """the drop-in UNet (f32) in the loop, x_T from the fixture: free-running over 19 evaluations the fp32 summation order of
    each eps separates the trajectories slightly (the PLMS test's bound), uint8 within 1 LSB"""
    v = load_npz("pndm.npz")
    m, _ = build_model("uf_label_c32_s16", "f32")
    d = _diffusion(m)
    x_T = torch.from_numpy(v["pndm10.x_T"])
    final, _ = d.sampler_list["pndm"].sample(shape=(B, 3, S, S), sampling_kwargs=_skw(10), denoise_sample_fn=d.denoise_sample_fn,
                                             denoise_sample_fn_kwargs=_dkw(), x_T=x_T)
    r = rel_l2(final.cpu(), v["pndm10.final"])
    samples, inter = d.p_sample_loop("pndm", (B, 3, S, S), _skw(10), denoise_sample_fn_kwargs=_dkw(), condition_kwargs={},
                                     x_T=x_T)
    du8 = (samples.cpu().int() - torch.from_numpy(v["pndm10.samples_u8"]).int()).abs()
    print(f"pndm10 free-running: rel_l2 {r:.3e}, u8 max diff {int(du8.max())}, u8 differing {float((du8 > 0).float().mean()):.2e}")
    assert r < 5e-3
    assert du8.max() <= 1


def _count_replays(monkeypatch):
    from sgdm_amd import diffusion as Dm
    count = [0]
    orig = Dm._GraphedStep.step

    def step(self, *a, **k):
        count[0] += 1
        return orig(self, *a, **k)
    monkeypatch.setattr(Dm._GraphedStep, "step", step)
    return count


@pytest.mark.parametrize("name", ["uf_label_c32_s16", "ca_stego_c32_s16"])
def test_graph_captured_equals_eager(name, monkeypatch):
    from sgdm_amd.synth import synth_batch
    replays = _count_replays(monkeypatch)
    m, entry = build_model(name, "f16x3")
    d = _diffusion(m)
    kw = entry["ctor"]
    batch = synth_batch(kw["condition_method"], B, S, kw["cond_dim"], entry["layout_dim"], seed=23)
    cond = batch["cond"].cuda() if entry["kind"] == "unet_fast" else batch["cond"].float().cuda()
    dkw = dict(cond=cond, layout=batch["layout"].cuda() if "layout" in batch else None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(8))
    out = {}
    for graph in (False, True):
        torch.manual_seed(1234)
        final, _ = d.sampler_list["pndm"].sample(shape=(B, 3, S, S), sampling_kwargs=_skw(10, hip_graph=graph),
                                                 denoise_sample_fn=d.denoise_sample_fn, denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)
        torch.manual_seed(1234)
        samples, _ = d.p_sample_loop("pndm", (B, 3, S, S), _skw(10, hip_graph=graph), denoise_sample_fn_kwargs=dict(dkw),
                                     condition_kwargs={}, x_T=x_T)
        out[graph] = (final.cpu(), samples.cpu())
        assert replays[0] == (38 if graph else 0)
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[False][0], out[True][0])
    assert torch.equal(out[False][1], out[True][1])


@pytest.mark.parametrize("graph", [True, False])
def test_rng_consumption_is_one_mask_draw_per_evaluation(graph):
    """per evaluation the reference draws only the UNet's cond-drop mask (uniform_ over 2B); the captured step draws no z"""
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion(m)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(9))
    run = lambda: d.p_sample_loop("pndm", (B, 3, S, S), _skw(10, hip_graph=graph), denoise_sample_fn_kwargs=_dkw(),
                                  condition_kwargs={}, x_T=x_T)
    run()                                       # engine, packed weights and the captured step built outside the count
    torch.manual_seed(77)
    run()
    got = torch.cuda.get_rng_state()
    torch.manual_seed(77)
    for _ in range(19):
        torch.empty(2 * B, device="cuda").uniform_()
    assert torch.equal(got, torch.cuda.get_rng_state())


@pytest.mark.parametrize("graph", [True, False])
def test_ignored_sampling_kwargs_and_return_value(graph):
    m, _ = build_model("uf_label_c32_s16", "f16x3")
    d = _diffusion(m)
    x_T = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    keep = x_T.clone()
    outs = []
    for extra in ({}, dict(clip_denoised=False, dtp=0.9, temperature=0.5, noise_dropout=0.1)):
        samples, inter = d.p_sample_loop("pndm", (B, 3, S, S), _skw(10, hip_graph=graph, **extra), denoise_sample_fn_kwargs=_dkw(),
                                         condition_kwargs={}, x_T=x_T)
        assert set(inter) == {"pred_x0"}
        assert inter["pred_x0"].dtype == torch.uint8 and tuple(inter["pred_x0"].shape) == (B, 3, S, S)
        assert torch.equal(inter["pred_x0"], samples)
        outs.append(samples.cpu())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(x_T, keep)


def test_c2_pndm50_captured_vs_torch_loop():
    """C2 shapes (unet_fast ch128, 64x64, bs 40 -> UNet batch 80, f16x3, w=2), PNDM-50 on the captured step, against the
    reference's algorithm restated in torch over the same HIP UNet's forward_with_cond_scale from the same x_T"""
    import bench
    wl = bench.WORKLOADS["c2"]
    m, _, data = bench.build_model(wl, "cuda", "f16x3")
    Bc, Sc = wl["batch"], wl["image"]
    d = _diffusion(m)
    dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(Bc, 3, Sc, Sc, generator=torch.Generator().manual_seed(50)).cuda()
    final, _ = d.sampler_list["pndm"].sample(shape=(Bc, 3, Sc, Sc), sampling_kwargs=_skw(50), denoise_sample_fn=d.denoise_sample_fn,
                                             denoise_sample_fn_kwargs=dict(dkw), x_T=x_T)
    for eng in m._engines.values():
        eng.check_health()
    assert torch.isfinite(final).all()
    # pndm_sampler.py:13-211 restated: linear fp32 betas, alphas_cumprod + [0.0], lookups at t + 1
    T, n = 1000, 50
    betas = np.linspace(1e-4, 2e-2, T, dtype=np.float32)
    ac = torch.tensor(np.array(list(np.cumprod(1.0 - betas, axis=0)) + [0.0], dtype=np.float32), device="cuda")
    step = T // n
    times = list(range(0, T, step))
    warm = [int(t) for t in reversed((np.array(times[-4:]).repeat(2) + np.tile(np.array([0, step // 2]), 4))[:-1].repeat(2)[1:-1])]
    plms = list(reversed(times[:-3]))

    def transfer(x, t, t_next, et):
        at, an = ac[t + 1], ac[t_next + 1]
        return x + (an - at) * ((1 / (at.sqrt() * (at.sqrt() + an.sqrt()))) * x
                                - 1 / (at.sqrt() * (((1 - an) * at).sqrt() + ((1 - at) * an).sqrt())) * et)

    def eps(x, t):
        return m.forward_with_cond_scale(x, torch.full((Bc,), int(t), device="cuda", dtype=torch.long), **dkw)

    with torch.no_grad():
        x, ets, acc, base = x_T.clone(), [], 0, None
        for j, t in enumerate(warm):
            e = eps(x, t)
            tp, tn = warm[j // 4 * 4], warm[min(j + 1, 11)]
            if j % 4 == 0:
                acc, base = acc + 1 / 6 * e, x
                ets.append(e)
            elif j % 4 in (1, 2):
                acc = acc + 1 / 3 * e
            else:
                e = acc + 1 / 6 * e
                acc = 0
            x = transfer(base, tp, tn, e)
        for k, t in enumerate(plms):
            ets.append(eps(x, t))
            r = (1 / 24) * (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4])
            x = transfer(x, t, plms[min(k + 1, len(plms) - 1)], r)
    r = rel_l2(final.cpu(), x.cpu())
    from sgdm_amd.diffusion import to_uint8
    du8 = (to_uint8(final).int() - to_uint8(x).int()).abs()
    print(f"C2 PNDM-50 captured vs torch loop: rel_l2 {r:.3e}, u8 max diff {int(du8.max())}")
    assert r < 1e-4
    assert du8.max() <= 1
