"""The sampling plan (sgdm_amd/sampling_plan.py: resolve_plan, SamplingPlan) on the host: its fields are what the option
functions return on the same kwargs, every refusal of theirs comes out of the resolver unchanged and before the library is
loaded, the record is frozen, and ``capture_key()`` splits trajectories into exactly the classes the captured-step cache key
had before the plan existed (written out below as pairs that share a capture and pairs that do not)."""
import dataclasses

import numpy as np
import pytest
import torch

from test_pag_cpu import _plan_model

DKW = dict(cond_scale=2.0)
T = 1000


@pytest.fixture(autouse=True)
def _no_load(monkeypatch):
    from sgdm_amd import _lib as L
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("library loaded")))


@pytest.fixture(scope="module")
def model():
    return _plan_model()                                    # scale_type 'imagen': mode 1


def _sk(**kw):
    return dict(dict(num_timesteps=10, clip_denoised=True, temperature=1.0, ddim_eta=1.0, log_num_per_prog=10), **kw)


# (kwargs, method, learned variance) -- each option alone, then the accepted pairs
ACCEPTED = [
    ({}, "ddim", False),
    (dict(cfg_rescale=0.7), "ddim", False),
    (dict(cfg_interval=(200, 800)), "pndm", False),
    (dict(cfg_distilled=True), "dpmsolver", False),
    (dict(pag_scale=1.5), "plms", False),
    (dict(pag_scale=1.5, pag_layers="all", pag_drop_cond=True), "ddim", False),
    (dict(parameterization="v"), "ddim", False),
    (dict(parameterization="v", v_form="data"), "dpmsolver", False),
    (dict(parameterization="x0"), "native", False),
    (dict(native_steps=10), "native", False),
    ({}, "native", True),
    (dict(dtp=0.9), "ddim", False),
    (dict(noise_dropout=0.25), "native", False),
    (dict(hip_graph=False), "ddim", False),
    (dict(clip_denoised=False), "ddim", False),
    (dict(cfg_interval=(200, 800), cfg_rescale=0.7), "native", False),
    (dict(pag_scale=1.5, cfg_interval=(200, 800)), "ddim", False),
    (dict(parameterization="v", v_form="data", cfg_rescale=0.3), "native", False),
    (dict(native_steps=10), "native", True),
    (dict(parameterization="v", native_steps=7, pag_scale=2), "native", True),
]


@pytest.mark.parametrize("opt,method,lv", ACCEPTED)
def test_fields_are_what_the_leaf_functions_return(opt, method, lv, model):
    from sgdm_amd import sampling_plan as P
    sk = _sk(**opt)
    plan = P.resolve_plan(sk, method, model, DKW, T=T, lv=lv)
    fused = True                                            # the drop-in model, a float weight that is no shortcut, no p0
    assert plan.fused is fused and plan.method == method and plan.lv is lv
    assert (plan.rescale, plan.interval) == P.cfg_options(sk, fused)
    assert plan.scheduled == (plan.rescale > 0 or plan.interval is not None)
    assert plan.distilled == P.cfg_distilled_option(sk)
    assert plan.pag == P.pag_options(sk, fused, model)
    assert plan.layers == (plan.pag[1] if plan.pag else None)
    assert plan.form == P.v_form_option(sk, method) and plan.par == opt.get("parameterization", "eps")
    assert plan.native_steps == P.native_steps_option(sk, method, T)
    assert plan.mode == (2 if plan.pag else 1)
    assert plan.weight == (plan.pag[0] if plan.pag else None if plan.distilled else 2.0)
    assert (plan.dtp, plan.noise_dropout) == (opt.get("dtp", 1), opt.get("noise_dropout", 0))
    assert plan.clip == (0 if method == "pndm" else int(sk["clip_denoised"])) and plan.hip_graph is opt.get("hip_graph", True)
    if plan.scheduled:
        times = [999, 800, 500, 200, 199, 0]
        assert plan.schedule(times) == P.cfg_schedule(times, plan.weight, plan.mode, plan.interval)


def test_defaults_of_a_bare_step_and_of_a_generic_function(model):
    from sgdm_amd import sampling_plan as P
    bare = P.resolve_plan(None)
    assert bare == P.SamplingPlan(method=None, par="eps", form="eps", rescale=0.0, interval=None, scheduled=False, distilled=False,
                                  pag=None, lv=False, native_steps=None, dtp=1, noise_dropout=0, clip=0, hip_graph=True,
                                  fused=False, mode=None, weight=None)
    # the single-evaluation shortcuts, p0 and a tensor weight are not the fused step; neither is a generic function
    for m, kw in ((model, dict(cond_scale=1.0)), (model, dict(cond_scale=0)), (model, dict(cond_scale=2.0, p0=torch.zeros(1))),
                  (model, dict(cond_scale=torch.ones(1, 1, 1, 1))), (None, DKW)):
        plan = P.resolve_plan(_sk(), "ddim", m, kw, T=T)
        assert not plan.fused and plan.mode is None and plan.weight is None
    assert P.resolve_plan(_sk(cfg_distilled=True), "ddim", model, {}, T=T).fused          # cond_scale is not read
    assert P.resolve_plan(_sk(pag_scale=1.0), "ddim", model, {}, T=T).weight == 1.0        # likewise
    # the schedule's parameterization stands in where the kwargs leave it out, and only there
    assert P.resolve_plan(_sk(), "native", model, DKW, T=T, par="v").par == "v"
    assert P.resolve_plan(_sk(parameterization="eps"), "native", model, DKW, T=T, par="v").par == "eps"
    # the environment switch is part of the plan
    import os
    from unittest import mock
    with mock.patch.dict(os.environ, dict(SGDM_HIP_GRAPH="0")):
        assert not P.resolve_plan(_sk(), "ddim", model, DKW, T=T).hip_graph


ZERO = np.asarray([0.5, 0.0])

# (kwargs, method, learned variance, visited alphas_cumprod, the leaf call that raises the same)
REFUSED = [
    (dict(cfg_rescale=1.5), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_rescale=True), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_interval=(5, 1)), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_interval=(0.0, 5)), "pndm", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_distilled=1), "ddim", False, None, lambda P, sk, m: P.cfg_distilled_option(sk)),
    (dict(cfg_distilled=True, cfg_rescale=0.5), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_distilled=True, cfg_interval=(0, 5)), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(cfg_distilled=True), "native", True, None, lambda P, sk, m: P.cfg_options(dict(sk, lv_native=True), True)),
    (dict(cfg_distilled=True, lv_native=True), "ddim", False, None, lambda P, sk, m: P.cfg_options(sk, True)),
    (dict(pag_scale=-0.1), "ddim", False, None, lambda P, sk, m: P.pag_scale_option(sk)),
    (dict(pag_scale=True), "ddim", False, None, lambda P, sk, m: P.pag_scale_option(sk)),
    (dict(pag_layers="all"), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(pag_drop_cond=True), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(pag_scale=1.0, cfg_distilled=True), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(pag_scale=1.0, pag_layers="middle"), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(pag_scale=1.0, pag_layers=["middle_block.0"]), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(pag_scale=1.0, pag_drop_cond=1), "ddim", False, None, lambda P, sk, m: P.pag_options(sk, True, m)),
    (dict(v_form="velocity"), "ddim", False, None, lambda P, sk, m: P.v_form_option(sk, "ddim")),
    (dict(v_form="data"), "ddim", False, None, lambda P, sk, m: P.v_form_option(sk, "ddim")),
    (dict(parameterization="v", v_form="data", dtp=0.9), "ddim", False, None, lambda P, sk, m: P.v_form_option(sk, "ddim")),
    (dict(parameterization="v", v_form="data"), "plms", False, None, lambda P, sk, m: P.v_form_option(sk, "plms")),
    (dict(parameterization="v", v_form="data"), "pndm", False, None, lambda P, sk, m: P.v_form_option(sk, "pndm")),
    (dict(parameterization="v"), "ddim", False, ZERO, lambda P, sk, m: P.v_form_option(sk, "ddim", ZERO)),
    (dict(), "plms", False, ZERO, lambda P, sk, m: P.v_form_option(sk, "plms", ZERO)),
    (dict(native_steps=10), "ddim", False, None, lambda P, sk, m: P.native_steps_option(sk, "ddim", T)),
    (dict(native_steps=10), "pndm", False, None, lambda P, sk, m: P.native_steps_option(sk, "pndm", T)),
    (dict(native_steps=1), "native", False, None, lambda P, sk, m: P.native_steps_option(sk, "native", T)),
    (dict(native_steps=T + 1), "native", False, None, lambda P, sk, m: P.native_steps_option(sk, "native", T)),
    (dict(native_steps=10.0), "native", False, None, lambda P, sk, m: P.native_steps_option(sk, "native", T)),
    (dict(dtp=0.9), "native", True, None, lambda P, sk, m: P.lv_native_option(sk)),
    (dict(noise_dropout=0.1), "native", True, None, lambda P, sk, m: P.lv_native_option(sk)),
    (dict(cfg_interval=(0, 5)), "native", True, None, lambda P, sk, m: P.lv_native_option(sk)),
    (dict(cfg_rescale=0.5), "native", True, None, lambda P, sk, m: P.lv_native_option(sk)),
    (dict(parameterization="v", v_form="data"), "native", True, None, lambda P, sk, m: P.lv_native_option(sk)),
]


@pytest.mark.parametrize("opt,method,lv,visited,leaf", REFUSED)
def test_every_refusal_of_the_leaf_functions_comes_out_unchanged(opt, method, lv, visited, leaf, model):
    from sgdm_amd import sampling_plan as P
    sk = _sk(**opt)
    with pytest.raises(ValueError) as want:
        leaf(P, sk, model)
    with pytest.raises(ValueError) as got:
        P.resolve_plan(sk, method, model, DKW, T=T, ac_visited=visited, lv=lv)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)


def test_refusals_that_depend_on_the_step_and_on_later_knowledge(model):
    from sgdm_amd import sampling_plan as P
    generic = [(dict(cfg_rescale=0.5), lambda sk: P.cfg_options(sk, False)),
               (dict(cfg_interval=(0, 5)), lambda sk: P.cfg_options(sk, False)),
               (dict(cfg_distilled=True), lambda sk: P.cfg_options(sk, False)),
               (dict(pag_scale=1.0), lambda sk: P.pag_options(sk, False, None))]
    for opt, leaf in generic:
        sk = _sk(**opt)
        with pytest.raises(ValueError) as want:
            leaf(sk)
        for m, kw in ((None, DKW), (model, dict(cond_scale=2.0, p0=torch.zeros(1)))):
            with pytest.raises(ValueError) as got:
                P.resolve_plan(sk, "ddim", m, kw, T=T)
            assert str(got.value) == str(want.value)
    # a sampler whose times follow from the plan hands the visited entries over afterwards: the same refusal
    plan = P.resolve_plan(_sk(parameterization="v"), "dpmsolver", model, DKW, T=T)
    with pytest.raises(ValueError) as want:
        P.v_form_option(_sk(parameterization="v"), "dpmsolver", ZERO)
    with pytest.raises(ValueError) as got:
        plan.visits(ZERO)
    assert str(got.value) == str(want.value)
    assert plan.visits(np.asarray([0.5, 0.1])) is plan
    data = P.resolve_plan(_sk(parameterization="v", v_form="data"), "dpmsolver", model, DKW, T=T)
    assert data.visits(ZERO) is data                        # the data form is finite there


def test_the_samplers_refuse_through_the_plan_before_the_load():
    """end to end: a sampler's ``sample`` raises the resolver's refusal, the denoise function is never called and the
    library never asked for (the autouse fixture turns a load into an AssertionError)"""
    import bench
    from sgdm_amd import diffusion as Dm
    d = Dm.LatentDiffusion(device="cpu", **bench.MODEL_PARAMS)
    called = []
    fn = lambda x, t, **k: called.append(1) or x
    for method, opt, msg in (("native", dict(num_timesteps=T, native_steps=1), "native_steps"),
                             ("ddim", dict(native_steps=10), "native_steps"), ("pndm", dict(v_form="data"), "v_form"),
                             ("dpmsolver", dict(cfg_rescale=0.5), "fused-CFG"), ("plms", dict(pag_scale=1.0), "pag_scale")):
        with pytest.raises(ValueError, match=msg):
            d.sampler_list[method].sample(shape=(1, 3, 4, 4), sampling_kwargs=_sk(alphas_cumprod=d.sampler.alphas_cumprod, **opt),
                                          denoise_sample_fn=fn, denoise_sample_fn_kwargs=dict(DKW), x_T=torch.zeros(1, 3, 4, 4))
    with pytest.raises(AssertionError, match="library loaded"):                 # accepted: goes on to load the library
        d.sampler_list["ddim"].sample(shape=(1, 3, 4, 4), sampling_kwargs=_sk(alphas_cumprod=d.sampler.alphas_cumprod),
                                      denoise_sample_fn=fn, denoise_sample_fn_kwargs=dict(DKW), x_T=torch.zeros(1, 3, 4, 4))
    assert not called


def test_the_plan_is_frozen(model):
    from sgdm_amd import sampling_plan as P
    plan = P.resolve_plan(_sk(cfg_rescale=0.5), "ddim", model, DKW, T=T)
    for f in dataclasses.fields(plan):
        with pytest.raises(dataclasses.FrozenInstanceError):
            setattr(plan, f.name, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.extra = 1
    hash(plan.capture_key())                                # the key is hashable: it goes into a dict


# ------------------------------------------------------------------------------------------- capture-key classes
# The captured-step cache key, as _GraphedStep.get assembled it by hand before the plan: (engine, image shape, update kind,
# clip, temperature, w -- None on a scheduled or distilled step, else the static weight --, mode, cond / layout signatures,
# 'eps' | ('v', n) | ('v', n, 'data'), (rescale, an interval is given), (lv, head, native_steps), distilled, PAG's (layers,
# drop_cond)).  Of these the plan owns w, mode, the 'v' kind, rescale, whether an interval is given, lv, distilled and the
# PAG pair; the pairs below follow from that list, option by option.  Each entry: (kwargs, denoise kwargs, learned variance).

V = dict(parameterization="v")
SHARE = [
    ((dict(cfg_rescale=0.7), dict(cond_scale=2.0), False), (dict(cfg_rescale=0.7), dict(cond_scale=3.0), False)),
    ((dict(cfg_interval=(200, 800)), DKW, False), (dict(cfg_interval=(0, 100)), DKW, False)),
    ((dict(cfg_interval=(200, 800)), dict(cond_scale=2.0), False), (dict(cfg_interval=(200, 800)), dict(cond_scale=5.0), False)),
    ((dict(pag_scale=1.5, cfg_rescale=0.7), DKW, False), (dict(pag_scale=3.0, cfg_rescale=0.7), DKW, False)),
    ((dict(pag_scale=1.5, cfg_interval=(200, 800)), DKW, False), (dict(pag_scale=0.5, cfg_interval=(1, 2)), DKW, False)),
    ((dict(cfg_distilled=True), dict(cond_scale=2.0), False), (dict(cfg_distilled=True), dict(cond_scale=7.0), False)),
    ((dict(pag_scale=1.5), dict(cond_scale=2.0), False), (dict(pag_scale=1.5), dict(cond_scale=9.0), False)),
    # what the plan carries but the capture does not bake in: the eager-only switches stay out of the key
    ((dict(), DKW, False), (dict(hip_graph=True, dtp=1, noise_dropout=0), DKW, False)),
    ((dict(parameterization="x0"), DKW, False), (dict(), DKW, False)),       # read as eps: no tables, no conversion
    ((V, DKW, True), (dict(), DKW, True)),                                      # the learned-variance update converts nothing
]
SPLIT = [
    ((dict(), dict(cond_scale=2.0), False), (dict(), dict(cond_scale=3.0), False)),
    ((dict(), DKW, False), (V, DKW, False)),
    ((V, DKW, False), (dict(V, v_form="data"), DKW, False)),
    ((dict(), DKW, False), (dict(V, v_form="data"), DKW, False)),
    ((dict(), DKW, False), (dict(cfg_distilled=True), DKW, False)),
    ((dict(pag_scale=1.5, pag_layers="mid"), DKW, False), (dict(pag_scale=1.5, pag_layers="all"), DKW, False)),
    ((dict(pag_scale=1.5, pag_drop_cond=True), DKW, False), (dict(pag_scale=1.5, pag_drop_cond=False), DKW, False)),
    ((dict(pag_scale=1.5), DKW, False), (dict(pag_scale=2.5), DKW, False)),   # unscheduled: a static weight
    ((dict(pag_scale=2.0), DKW, False), (dict(), DKW, False)),                # same weight 2.0: the mode and the layers differ
    ((dict(), DKW, True), (dict(), DKW, False)),
    ((dict(cfg_rescale=0.3), DKW, False), (dict(cfg_rescale=0.7), DKW, False)),
    ((dict(cfg_interval=(200, 800)), DKW, False), (dict(), DKW, False)),
    ((dict(cfg_interval=(200, 800), cfg_rescale=0.7), DKW, False), (dict(cfg_rescale=0.7), DKW, False)),
    ((dict(cfg_rescale=0.7), DKW, False), (dict(), DKW, False)),
]


def _key(case, model):
    from sgdm_amd.sampling_plan import resolve_plan
    opt, dkw, lv = case
    return resolve_plan(_sk(num_timesteps=T, **opt), "native", model, dkw, T=T, lv=lv).capture_key()


@pytest.mark.parametrize("a,b", SHARE)
def test_trajectories_that_share_a_captured_step(a, b, model):
    assert _key(a, model) == _key(b, model)


@pytest.mark.parametrize("a,b", SPLIT)
def test_trajectories_that_do_not(a, b, model):
    assert _key(a, model) != _key(b, model)


def test_scale_type_is_part_of_the_key():
    imagen, cfg = _plan_model(), _plan_model()
    cfg.condition["scale_type"] = "cfg"
    assert _key((dict(), DKW, False), imagen) != _key((dict(), DKW, False), cfg)


def test_the_update_states_its_part_of_the_key(model, monkeypatch):
    """kind, clip, temperature and native_steps: the update's own, known at construction"""
    from sgdm_amd import _lib as L
    from sgdm_amd import diffusion as Dm
    from sgdm_amd.sampling_plan import resolve_plan
    monkeypatch.setattr(L, "load", lambda: None)            # (an update keeps the library handle; nothing is launched)
    plan = resolve_plan(_sk(num_timesteps=T, native_steps=10), "native", model, DKW, T=T)
    assert Dm._DDUpdate("ddpm", plan).capture_key() == ("ddpm", 1, 1.0, 10)
    plain = resolve_plan(_sk(clip_denoised=False), "ddim", model, DKW, T=T)
    assert Dm._DDUpdate("ddim", plain, 0.5).capture_key() == ("ddim", 0, 0.5, None)
    assert Dm._VUpdate("v_dpmsolver", plain, noise=False).capture_key() == ("v_dpmsolver", 0, 1.0, None)
    assert Dm._PNDMUpdate("pndm", resolve_plan(_sk(), "pndm", model, DKW, T=T)).capture_key() == ("pndm", 0, 1.0, None)
    # whether a step is captured at all: one predicate of plan and update
    upd = Dm._DDUpdate("ddim", plain)
    assert plain.captured(upd) and not plain.captured(upd, capture=False)
    for opt in (dict(hip_graph=False), dict(dtp=0.9), dict(noise_dropout=0.25)):
        p = resolve_plan(_sk(**opt), "ddim", model, DKW, T=T)
        assert not p.captured(Dm._DDUpdate("ddim", p))
    p = resolve_plan(_sk(noise_dropout=0.25), "dpmsolver", model, DKW, T=T)
    assert p.captured(Dm._DPMUpdate("dpmsolver", p))        # an update that does not honour the extras never sees them
    generic = resolve_plan(_sk(), "ddim", None, DKW, T=T)
    assert not generic.captured(Dm._DDUpdate("ddim", generic))
