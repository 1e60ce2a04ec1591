"""parameterization='v' (Salimans & Ho 2022: v = sqrt(ac_t) * noise - sqrt(1 - ac_t) * x_start) on the host side: the
diffusion object constructs, p_losses forms the v target, p_sample_loop tells the sampler.  The reference has no such
parameterization; the expected values are the formula restated in float64.  No GPU."""
import numpy as np
import pytest
import torch


def _params(**kw):
    import bench
    return dict(bench.MODEL_PARAMS, parameterization="v", **kw)


def test_v_objects_construct_on_cpu():
    from sgdm_amd.diffusion import LatentDiffusion, Schedule_DDPM
    d = LatentDiffusion(device="cpu", **_params())
    s = Schedule_DDPM(device="cpu", **_params())
    for sched in (d.sampler, s):
        assert sched.hparams.parameterization == "v"
        assert sched.lvlb_weights.shape == (1000,) and torch.isfinite(sched.lvlb_weights).all()
    # the eps expression stands in (no loss path reads it)
    e = Schedule_DDPM(device="cpu", **dict(_params(), parameterization="eps"))
    assert torch.equal(s.lvlb_weights, e.lvlb_weights)
    with pytest.raises(NotImplementedError):
        Schedule_DDPM(device="cpu", **dict(_params(), parameterization="mu"))


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
def test_p_losses_target_is_v(loss_type):
    """a denoise_fn returning a fixed tensor: the loss is that of the float64 restatement of v, within fp32 rounding"""
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cpu", **_params(loss_type=loss_type)).train()
    g = torch.Generator().manual_seed(7)
    B = 4
    x0 = torch.randn(B, 3, 8, 8, generator=g)
    noise = torch.randn(B, 3, 8, 8, generator=g)
    out = torch.randn(B, 3, 8, 8, generator=g)
    t = torch.tensor([0, 999, 500, 37])
    seen = {}

    def denoise_fn(x_noisy, tt, **kw):
        seen["x_noisy"], seen["t"] = x_noisy, tt
        return out, 0.0, dict()

    d.set_denoise_fn(denoise_fn, None)
    loss, ld = d.p_losses(x0, t, noise)
    # the schedule in float64 (the fp32 alphas_cumprod buffer is too coarse for 1 - ac at small t)
    from sgdm_amd.diffusion import make_beta_schedule
    h = d.hparams
    ac = torch.from_numpy(np.cumprod(1.0 - make_beta_schedule(h.beta_schedule, h.num_timesteps, h.linear_start, h.linear_end)))
    sa, s1 = ac.sqrt()[t].view(B, 1, 1, 1), (1 - ac).sqrt()[t].view(B, 1, 1, 1)
    assert torch.allclose(seen["x_noisy"].double(), sa * x0.double() + s1 * noise.double(), rtol=1e-6, atol=1e-6)
    v = sa * noise.double() - s1 * x0.double()
    diff = v - out.double()
    if loss_type == "l2":
        per = (diff ** 2).reshape(B, -1).mean(1)
    elif loss_type == "l1":
        per = diff.abs().reshape(B, -1).mean(1)
    else:
        per = torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5).reshape(B, -1).mean(1)
    assert torch.allclose(loss.double(), per.mean(), rtol=1e-6, atol=0)
    assert torch.allclose(ld["train/epoch_stats_y"].double(), per, rtol=1e-6, atol=0)
    assert sorted(ld) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    # and it is not the eps or x0 loss
    assert not torch.allclose(loss.double(), ((noise - out).double() ** 2).mean(), rtol=1e-3)


@pytest.mark.parametrize("par", ["v", "eps", "x0"])
def test_p_sample_loop_tells_the_sampler_the_parameterization(par):
    from sgdm_amd.diffusion import LatentDiffusion
    d = LatentDiffusion(device="cpu", **dict(_params(), parameterization=par))
    d.set_denoise_fn(None, lambda x, t, **kw: x)
    got = {}

    class Stub:
        def sample(self, shape, sampling_kwargs, denoise_sample_fn, **kwargs):
            got.update(sampling_kwargs)
            img = torch.zeros(shape)
            return img, dict(pred_x0=img.clone())

    d.sampler_list["stub"] = Stub()
    caller = dict(num_timesteps=5)
    samples, _ = d.p_sample_loop("stub", (1, 3, 4, 4), caller, condition_kwargs={})
    assert samples.dtype == torch.uint8
    assert got["parameterization"] == par
    assert got["alphas_cumprod"] is d.sampler.alphas_cumprod
    if par == "v":      # the tables of the v -> eps pass are the training schedule's
        assert got["sqrt_alphas_cumprod"] is d.sampler.sqrt_alphas_cumprod
        assert got["sqrt_one_minus_alphas_cumprod"] is d.sampler.sqrt_one_minus_alphas_cumprod
    assert caller == dict(num_timesteps=5)      # the caller's dict is not written to


def test_direct_sampler_call_defaults_to_eps():
    from sgdm_amd.diffusion import _v_tables
    ac = torch.linspace(0.999, 0.001, 10)
    assert _v_tables(dict(alphas_cumprod=ac), "cpu") is None
    assert _v_tables(dict(alphas_cumprod=ac, parameterization="x0"), "cpu") is None
    sa, s1 = _v_tables(dict(alphas_cumprod=ac, parameterization="v"), "cpu")
    assert sa.dtype == s1.dtype == torch.float32
    assert torch.equal(sa, ac.double().sqrt().float()) and torch.equal(s1, (1 - ac.double()).sqrt().float())
    with pytest.raises(NotImplementedError):
        _v_tables(dict(alphas_cumprod=ac, parameterization="mu"), "cpu")
