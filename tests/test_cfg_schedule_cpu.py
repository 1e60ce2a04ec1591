"""Guidance schedule (sampling kwargs cfg_interval / cfg_rescale, sgdm_amd/diffusion.py) where it needs no GPU: the host table
of guided / cond-only evaluations, the argument checks -- raised before the library is loaded -- and the binding of the guide
pass (include/sgdm_hip.h: sgd_cfg_guide)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT


def test_table_on_ddim_uniform_times_both_scale_modes():
    from sgdm_amd.diffusion import cfg_schedule, make_ddim_timesteps
    times = make_ddim_timesteps("uniform", 10, 1000)            # 1, 101, .., 901
    assert list(times) == list(range(1, 1000, 100))
    g, w = cfg_schedule(times, 2.5, 1, (301, 601))              # imagen form: cond-only is weight 1
    assert g == [False] * 3 + [True] * 4 + [False] * 3
    assert w == [1.0] * 3 + [2.5] * 4 + [1.0] * 3
    g2, w2 = cfg_schedule(times, 2.5, 2, (301, 601))            # cfg form: cond-only is weight 0
    assert g2 == g and w2 == [0.0] * 3 + [2.5] * 4 + [0.0] * 3
    with pytest.raises(ValueError):
        cfg_schedule(times, 2.5, 0, None)


def test_table_bounds_are_inclusive_and_in_training_timesteps():
    from sgdm_amd.diffusion import cfg_schedule
    times = [1, 101, 201, 301]
    assert cfg_schedule(times, 3, 2, (101, 201))[0] == [False, True, True, False]
    assert cfg_schedule(times, 3, 2, (102, 200))[0] == [False] * 4
    assert cfg_schedule(times, 3, 2, (201, 201))[0] == [False, False, True, False]
    assert cfg_schedule(times, 3, 2, (0, 1))[0] == [True, False, False, False]
    g, w = cfg_schedule(np.asarray(times), 3, 2, (0, 999))      # numpy times, int weight
    assert g == [True] * 4 and w == [3.0] * 4 and all(isinstance(v, float) for v in w)


def test_table_none_guides_everything_and_an_interval_may_hit_nothing():
    from sgdm_amd.diffusion import cfg_schedule
    times = list(range(1, 1000, 100))
    g, w = cfg_schedule(times, 2.0, 1, None)
    assert g == [True] * 10 and w == [2.0] * 10
    g, w = cfg_schedule(times, 2.0, 1, (2, 100))
    assert g == [False] * 10 and w == [1.0] * 10
    g, w = cfg_schedule(times, 2.0, 2, (2, 100))
    assert g == [False] * 10 and w == [0.0] * 10
    assert cfg_schedule([], 2.0, 2, (0, 10)) == ([], [])


def test_table_judges_every_pndm_evaluation_by_its_own_time():
    """PNDM's list has one entry per UNet EVALUATION: the Runge-Kutta warm-up repeats times and visits half steps"""
    from sgdm_amd.diffusion import PNDM_Sampler, cfg_schedule
    times, tab = PNDM_Sampler(1000, 1e-4, 2e-2, device="cpu").plan(10)
    assert len(times) == len(tab) == 12 + 7 and len(set(times)) < len(times)
    g, w = cfg_schedule(times, 2.0, 2, (300, 650))
    assert g == [300 <= t <= 650 for t in times]
    assert 0 < sum(g) < len(g)
    assert any(a == b and ga == gb for (a, ga), (b, gb) in zip(zip(times, g), zip(times[1:], g[1:])))   # a repeated time, one verdict
    assert w == [2.0 if f else 0.0 for f in g]
    # a half-step time (t + 50) inside, its neighbours outside
    half = [t for t in times if t % 100 == 50]
    assert half, times
    g, _ = cfg_schedule(times, 2.0, 2, (half[0], half[0]))
    assert [t for t, f in zip(times, g) if f] == [half[0]] * times.count(half[0])


def test_options_are_validated():
    from sgdm_amd.diffusion import cfg_options
    assert cfg_options(None) == (0.0, None) and cfg_options({}) == (0.0, None)
    assert cfg_options(dict(cfg_rescale=0.7, cfg_interval=(200, 800))) == (0.7, (200, 800))
    assert cfg_options(dict(cfg_rescale=1, cfg_interval=[np.int64(5), 5])) == (1.0, (5, 5))
    assert cfg_options(dict(cfg_rescale=0, cfg_interval=None), fused=False) == (0.0, None)      # nothing set: nothing to refuse
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError):
            cfg_options(dict(cfg_rescale=bad))
    for bad in ((3,), (1, 2, 3), (1.0, 2), (2, 1), "ab", 5, (True, 2), (None, 4)):
        with pytest.raises(ValueError):
            cfg_options(dict(cfg_interval=bad))
    for sk in (dict(cfg_rescale=0.5), dict(cfg_interval=(0, 999)), dict(cfg_rescale=1.0, cfg_interval=(3, 4))):
        with pytest.raises(ValueError, match="fused-CFG"):
            cfg_options(sk, fused=False)


def _sk(**kw):
    ac = torch.linspace(0.9999, 0.01, 1000)
    return dict(dict(num_timesteps=10, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1, temperature=1.0,
                     noise_dropout=0, alphas_cumprod=ac, vis=None), **kw)


@pytest.mark.parametrize("method", ["ddim", "plms", "pndm", "dpmsolver"])
@pytest.mark.parametrize("opt,msg", [(dict(cfg_rescale=0.5), "fused-CFG"), (dict(cfg_interval=(100, 500)), "fused-CFG"),
                                     (dict(cfg_rescale=2.0), "cfg_rescale"), (dict(cfg_interval=(500, 100)), "cfg_interval"),
                                     (dict(cfg_interval=(1.5, 100)), "cfg_interval")])
def test_samplers_refuse_before_the_library_is_loaded(method, opt, msg, monkeypatch):
    """a generic denoise_sample_fn is not the fused-CFG step; malformed options are refused whatever the step"""
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm

    def no_load():
        raise AssertionError("the library was loaded before the options were checked")
    monkeypatch.setattr(L, "load", no_load)
    s = dict(ddim=lambda: Dm.DDIMSampler(1000, "cpu", "ddim"), plms=lambda: Dm.DDIMSampler(1000, "cpu", "plms"),
             pndm=lambda: Dm.PNDM_Sampler(1000, 1e-4, 2e-2, device="cpu"), dpmsolver=lambda: Dm.DPMSolverSampler(1000, "cpu"))[method]()
    called = []
    fn = lambda x, t, **k: called.append(1) or x
    with pytest.raises(ValueError, match=msg):
        s.sample(shape=(1, 3, 4, 4), sampling_kwargs=_sk(**opt), denoise_sample_fn=fn,
                 denoise_sample_fn_kwargs=dict(cond_scale=2.0), x_T=torch.zeros(1, 3, 4, 4))
    assert not called


def test_native_sampler_and_the_non_fused_kinds_of_step_refuse(monkeypatch):
    import bench
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))
    d = Dm.LatentDiffusion(device="cpu", **bench.MODEL_PARAMS)
    sk = dict(_sk(cfg_interval=(100, 500), num_timesteps=1000), alphas_cumprod=d.sampler.alphas_cumprod)
    with pytest.raises(ValueError, match="fused-CFG"):
        d.sampler.sample((1, 3, 4, 4), sampling_kwargs=sk, denoise_sample_fn=lambda x, t, **k: x,
                         denoise_sample_fn_kwargs=dict(cond_scale=2.0), x_T=torch.zeros(1, 3, 4, 4))
    # p_sample_loop hands the two keys on unchanged
    d.set_denoise_fn(None, lambda x, t, **k: x)
    with pytest.raises(ValueError, match="fused-CFG"):
        d.p_sample_loop("ddim", (1, 3, 4, 4), _sk(cfg_rescale=0.5), denoise_sample_fn_kwargs=dict(cond_scale=2.0),
                        x_T=torch.zeros(1, 3, 4, 4))
    # the kinds of step SamplingPlan.fused says no to, on (a stand-in for) the drop-in UNet
    from sgdm_amd.unet import UNetModelBase

    class Fake(UNetModelBase):
        KIND = "unet_fast"

        def __init__(self):
            torch.nn.Module.__init__(self)
            self.condition = dict(scale_type="imagen")      # (the plan of an accepted step states how its halves are read)

        def forward_with_cond_scale(self, *a, **k):
            raise AssertionError("evaluated")

    m = Fake()
    assert Dm._unet_of(m.forward_with_cond_scale) is m
    for kw in (dict(cond_scale=torch.ones(1, 1, 1, 1)), dict(cond_scale=2.0, p0=torch.zeros(1)), dict(cond_scale=1.0),
               dict(cond_scale=0)):
        with pytest.raises(ValueError, match="fused-CFG"):
            Dm._StepRunner(m.forward_with_cond_scale, kw, dict(cfg_rescale=0.5))
    m.KIND = "unetca_fast"                              # int 0 / 1 only are its shortcuts
    with pytest.raises(ValueError, match="fused-CFG"):
        Dm._StepRunner(m.forward_with_cond_scale, dict(cond_scale=1), dict(cfg_interval=(0, 5)))
    with pytest.raises(AssertionError, match="library loaded"):                 # 1.0 is a fused weight there: accepted, goes on
        Dm._StepRunner(m.forward_with_cond_scale, dict(cond_scale=1.0), dict(cfg_interval=(0, 5)))


def test_binding_declares_the_guide_pass_and_the_abi_stays():
    import ctypes as C
    from sgdm_amd import _lib as L
    res, args = L.SIGNATURES["sgd_cfg_guide"]
    assert res is C.c_int32 and len(args) == 9 and args[3] is C.c_float and args[1] is C.c_int32
    txt = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    proto = re.search(r"int sgd_cfg_guide\(([^;]*)\);", txt).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == len(args)
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "guide.hip" in b._sources() and b.FILE_FLAGS["guide.hip"] == ["-ffp-contract=off"]
