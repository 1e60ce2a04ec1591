"""Loss weighting (hparam loss_weighting: 'min_snr', Hang et al. 2023; 'trunc_snr', Salimans & Ho 2022; 'p2', Choi et al. 2022;
'table') where it needs no GPU: the weight tables of sgdm_amd/diffusion.py: loss_weight_table against a float64 restatement,
the identities that tie the three parameterizations together, the refusals -- raised at construction, before the library is
loaded --, p_losses on the CPU with a stub denoiser, the unchanged path without the hparam, and the binding of the two new
entry points.  The reference weighs every timestep alike; the expected values are the published formulas restated here."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

T = 1000
SCHEDULES = {"linear": dict(beta_schedule="linear"), "cosine": dict(beta_schedule="cosine"),
             "zt": dict(beta_schedule="linear", zero_terminal_snr=True)}
SCHEMES = {"min_snr": dict(loss_weighting_gamma=5.0), "trunc_snr": {}, "p2": dict(loss_weighting_gamma=1.0, loss_weighting_k=1.0)}


def _diffusion(**kw):
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **dict(bench.MODEL_PARAMS, **kw))


# ('eps' on the zero-terminal schedule is refused by the schedule itself: tests/test_ztsnr_cpu.py)
TABLE_CASES = [(sched, par, scheme) for sched in sorted(SCHEDULES) for par in ("eps", "x0", "v") for scheme in sorted(SCHEMES)
               if not (sched == "zt" and par == "eps")]


def _omega(scheme, snr, gamma, k):
    """the weight on the x0 error, float64"""
    if scheme == "min_snr":
        return np.minimum(snr, gamma)
    if scheme == "trunc_snr":
        return np.maximum(snr, 1.0)
    return snr / (k + snr) ** gamma


def _want(ac32, par, scheme, gamma=5.0, k=1.0):
    """float64 restatement from the fp32 alphas_cumprod: omega, omega / SNR, omega / (SNR + 1); the 'eps' quotient at SNR == 0
    by its limit (min_snr: 1, p2: k^-gamma)"""
    a = ac32.double().numpy()
    snr = a / (1.0 - a)
    om = _omega(scheme, snr, gamma, k)
    if par == "x0":
        return om
    if par == "v":
        return om / (snr + 1.0)
    lim = dict(min_snr=1.0, p2=k ** -gamma).get(scheme, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(snr > 0, om / snr, lim)


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())


# ----------------------------------------------------------------------------------------------------------------- tables

@pytest.mark.parametrize("sched,par,scheme", TABLE_CASES)
def test_table_against_the_float64_restatement(sched, par, scheme):
    gamma = 1.0 if scheme == "p2" else 5.0
    d = _diffusion(parameterization=par, loss_weighting=scheme, **SCHEDULES[sched])            # default gamma / k
    s = d.sampler
    w = s.loss_weights
    assert w.dtype == torch.float32 and tuple(w.shape) == (T,) and torch.isfinite(w).all() and bool((w >= 0).all())
    assert "loss_weights" not in d.state_dict()                                                 # non-persistent
    want = _want(s.alphas_cumprod, par, scheme, gamma, 1.0)
    nz = want > 0
    assert _rel(w.numpy()[nz], want[nz]) <= 1e-6                # one fp32 rounding of a float64 value
    assert not w.numpy()[~nz].any()
    # explicit hparams give the same table; other values another one
    d2 = _diffusion(parameterization=par, loss_weighting=scheme, **SCHEDULES[sched], **SCHEMES[scheme])
    assert torch.equal(d2.sampler.loss_weights, w)
    if scheme != "trunc_snr":
        d3 = _diffusion(parameterization=par, loss_weighting=scheme, loss_weighting_gamma=2.0, loss_weighting_k=3.0,
                        **SCHEDULES[sched])
        want3 = _want(s.alphas_cumprod, par, scheme, 2.0, 3.0)
        nz3 = want3 > 0
        assert _rel(d3.sampler.loss_weights.numpy()[nz3], want3[nz3]) <= 1e-6
        assert not torch.equal(d3.sampler.loss_weights, w)


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("sched", ["linear", "cosine"])
def test_identities_across_parameterizations(sched, scheme):
    """w_eps * SNR == w_x0 == w_v * (SNR + 1) wherever SNR > 0"""
    from sgdm_amd.diffusion import loss_weight_table
    ac = _diffusion(**SCHEDULES[sched]).sampler.alphas_cumprod
    a = ac.double().numpy()
    snr = a / (1.0 - a)
    assert (snr > 0).all()
    gamma = 1.0 if scheme == "p2" else 5.0
    we, wx, wv = (loss_weight_table(ac, par, scheme, gamma, 1.0).double().numpy() for par in ("eps", "x0", "v"))
    assert _rel(we * snr, wx) <= 1e-6 and _rel(wv * (snr + 1.0), wx) <= 1e-6
    if scheme == "min_snr":
        assert (snr <= gamma).any() and (snr > gamma).any()
        assert (we[snr <= gamma] == 1.0).all() and (we[snr > gamma] < 1.0).all()


def test_zero_terminal_snr_weights():
    """the published formula gives the last timestep of a zero-terminal-SNR schedule no weight on 'v' and 'x0'"""
    for scheme in ("min_snr", "p2"):
        for par in ("v", "x0"):
            w = _diffusion(parameterization=par, zero_terminal_snr=True, loss_weighting=scheme).sampler.loss_weights
            assert float(w[-1]) == 0.0 and torch.isfinite(w).all() and bool((w[:-1] > 0).all()), (scheme, par)
    w = _diffusion(parameterization="v", zero_terminal_snr=True, loss_weighting="trunc_snr").sampler.loss_weights
    assert float(w[-1]) == 1.0 and torch.isfinite(w).all()                   # max(SNR, 1) / (SNR + 1) at SNR 0
    # 'table' is the way to a floor
    floor = _diffusion(parameterization="v", zero_terminal_snr=True, loss_weighting="min_snr").sampler.loss_weights.clamp_min(0.05)
    d = _diffusion(parameterization="v", zero_terminal_snr=True, loss_weighting="table", loss_weighting_table=floor)
    assert torch.equal(d.sampler.loss_weights, floor) and float(d.sampler.loss_weights[-1]) == pytest.approx(0.05)


def test_eps_quotients_are_finite_at_zero_snr():
    """the guard: 'eps' on a table that holds SNR == 0 (not constructible through the hparams)"""
    from sgdm_amd.diffusion import loss_weight_table
    ac = _diffusion(parameterization="v", zero_terminal_snr=True).sampler.alphas_cumprod
    assert float(ac[-1]) == 0.0
    assert float(loss_weight_table(ac, "eps", "min_snr", 5.0, 1.0)[-1]) == 1.0
    assert float(loss_weight_table(ac, "eps", "p2", 2.0, 4.0)[-1]) == pytest.approx(4.0 ** -2.0, rel=1e-6)
    with pytest.raises(ValueError, match="trunc_snr"):
        loss_weight_table(ac, "eps", "trunc_snr", 5.0, 1.0)
    one = ac.clone()
    one[0] = 1.0                                                # SNR = inf
    with pytest.raises(ValueError, match="not finite"):
        loss_weight_table(one, "x0", "trunc_snr", 5.0, 1.0)


# --------------------------------------------------------------------------------------------------------------- refusals

def _no_load(monkeypatch):
    from sgdm_amd import _lib as L

    def no_load():
        raise AssertionError("library loaded")
    monkeypatch.setattr(L, "load", no_load)


def test_refusals_at_construction_before_the_library_is_loaded(monkeypatch):
    _no_load(monkeypatch)
    ones = [1.0] * T
    bad = [(dict(loss_weighting="snr"), "loss_weighting"),
           (dict(loss_weighting="min_snr", loss_weighting_gamma=0.0), "gamma"),
           (dict(loss_weighting="min_snr", loss_weighting_gamma=-1.0), "gamma"),
           (dict(loss_weighting="p2", loss_weighting_gamma=float("nan")), "gamma"),
           (dict(loss_weighting="p2", loss_weighting_k=0.0), "loss_weighting_k"),
           (dict(loss_weighting="p2", loss_weighting_k=-2.0), "loss_weighting_k"),
           (dict(loss_weighting="table"), "loss_weighting_table"),
           (dict(loss_weighting="table", loss_weighting_table=ones[:-1]), "entries"),
           (dict(loss_weighting="table", loss_weighting_table=ones + [1.0]), "entries"),
           (dict(loss_weighting="table", loss_weighting_table=[-1.0] + ones[1:]), "non-negative"),
           (dict(loss_weighting="table", loss_weighting_table=[float("nan")] + ones[1:]), "finite"),
           (dict(loss_weighting="table", loss_weighting_table=[float("inf")] + ones[1:]), "finite"),
           (dict(loss_weighting="table", loss_weighting_table=[1e60] + ones[1:]), "finite"),
           (dict(loss_weighting_table=ones), "not 'table'"),
           (dict(loss_weighting="none", loss_weighting_table=ones), "not 'table'"),
           (dict(loss_weighting="min_snr", loss_weighting_table=ones), "not 'table'"),
           # a weight table that comes out non-finite: SNR = inf at alphas_cumprod == 1
           (dict(loss_weighting="trunc_snr", parameterization="x0", given_betas=np.concatenate([[0.0], np.linspace(1e-4, 2e-2, T - 1)])),
            "not finite")]
    from sgdm_amd.diffusion import Schedule_DDPM
    import bench
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            _diffusion(**kw)
        with pytest.raises(ValueError, match=match):
            Schedule_DDPM(device="cpu", **dict(bench.MODEL_PARAMS, **kw))
    # accepted, still without a library
    for kw in (dict(loss_weighting=None), dict(loss_weighting="none"), dict(loss_weighting="min_snr"), dict(loss_weighting="trunc_snr"),
               dict(loss_weighting="p2", loss_weighting_gamma=0.5, loss_weighting_k=2.0),
               dict(loss_weighting="table", loss_weighting_table=ones),
               dict(loss_weighting="table", loss_weighting_table=torch.ones(T)),
               dict(loss_weighting="table", loss_weighting_table=np.zeros(T))):
        _diffusion(**kw)


# ------------------------------------------------------------------------------------------------------ p_losses on the CPU

def _inputs(B=5):
    g = torch.Generator().manual_seed(19)
    x0, noise = torch.randn(B, 3, 8, 8, generator=g), torch.randn(B, 3, 8, 8, generator=g)
    out = 1.5 * torch.randn(B, 3, 8, 8, generator=g)            # |d| on both sides of huber's 1
    return x0, noise, out, torch.tensor([0, 999, 500, 37, 640])


def _per64(d, loss_type, par, x0, noise, out, t):
    """per-sample loss in float64 from the schedule's fp32 tables"""
    s, B = d.sampler, len(t)
    sa, s1 = s.sqrt_alphas_cumprod.double()[t].view(B, 1, 1, 1), s.sqrt_one_minus_alphas_cumprod.double()[t].view(B, 1, 1, 1)
    target = dict(eps=noise.double(), x0=x0.double(), v=sa * noise.double() - s1 * x0.double())[par]
    diff = out.double() - target
    if loss_type == "l2":
        el = diff ** 2
    elif loss_type == "l1":
        el = diff.abs()
    else:
        el = torch.where(diff.abs() < 1, 0.5 * diff ** 2, diff.abs() - 0.5)
    return el.reshape(B, -1).mean(1)


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("par,scheme", [("eps", "min_snr"), ("x0", "p2"), ("v", "min_snr"), ("v", "trunc_snr"), ("eps", "table")])
def test_p_losses_applies_the_weights(par, scheme, loss_type):
    extra = dict(loss_weighting_table=torch.linspace(0.0, 2.0, T)) if scheme == "table" else {}
    d = _diffusion(parameterization=par, loss_type=loss_type, loss_weighting=scheme, **extra).train()
    x0, noise, out, t = _inputs()
    d.set_denoise_fn(lambda x, tt, **kw: (out, 0.0, dict()), None)
    loss, ld = d.p_losses(x0, t, noise)
    per = _per64(d, loss_type, par, x0, noise, out, t)
    w = d.sampler.loss_weights.double()[t]
    assert len(set(w.tolist())) > 1
    want = (w * per).mean()
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want)
    assert sorted(ld) == ["train/ddpm_loss", "train/ddpm_loss_raw", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    assert torch.allclose(ld["train/epoch_stats_y"].double(), per, rtol=1e-6, atol=0)          # the UNWEIGHTED per-sample loss
    assert float(ld["train/ddpm_loss_raw"]) == pytest.approx(float(per.mean()), rel=1e-6)
    assert float(ld["train/ddpm_loss"]) == float(ld["train/loss"]) == float(loss)
    assert abs(float(loss) - float(per.mean())) > 1e-3 * float(per.mean())                     # and not the plain loss
    # validation: the val/ keys, no epoch_stats
    d.eval()
    with torch.no_grad():
        vloss, vd = d.p_losses(x0, t, noise)
    assert sorted(vd) == ["val/ddpm_loss", "val/ddpm_loss_raw", "val/loss"] and float(vloss) == float(loss)


@pytest.mark.parametrize("loss_type", ["l2", "l1", "huber"])
@pytest.mark.parametrize("par", ["eps", "x0", "v"])
def test_without_the_hparam_nothing_changes(par, loss_type):
    import bench
    assert not any(k.startswith("loss_weighting") for k in bench.MODEL_PARAMS)
    x0, noise, out, t = _inputs()
    runs = []
    for kw in ({}, dict(loss_weighting=None), dict(loss_weighting="none"), dict(loss_weighting="table", loss_weighting_table=[1.0] * T)):
        d = _diffusion(parameterization=par, loss_type=loss_type, **kw).train()
        d.set_denoise_fn(lambda x, tt, **k: (out, 0.0, dict()), None)
        runs.append(d.p_losses(x0, t, noise) + (d,))
    (loss, ld, d), (_, _, d_none), (_, _, d_off), (loss_1, ld_1, d_1) = runs[0], runs[1], runs[2], runs[3]
    for dd in (d, d_none, d_off):
        assert dd.sampler.loss_weighting is None and not hasattr(dd.sampler, "loss_weights")
        assert "loss_weights" not in dict(dd.sampler.named_buffers())
    assert sorted(ld) == ["train/ddpm_loss", "train/epoch_stats_x", "train/epoch_stats_y", "train/loss"]
    for other_loss, other_ld, _ in runs[1:3]:
        assert sorted(other_ld) == sorted(ld) and torch.equal(other_loss, loss)
        assert all(torch.equal(other_ld[k], ld[k]) for k in ld)
    # the restated plain loss, as before the feature
    per = _per64(d, loss_type, par, x0, noise, out, t)
    assert float(loss) == pytest.approx(float(per.mean()), rel=1e-6)
    # a table of ones weighs nothing: same value (x * 1.0 is exact), one more key
    assert torch.equal(loss_1, loss) and torch.equal(ld_1["train/epoch_stats_y"], ld["train/epoch_stats_y"])
    assert torch.equal(ld_1["train/ddpm_loss_raw"], ld["train/ddpm_loss"])


# ---------------------------------------------------------------------------------------------------------------- binding

def test_binding_declares_both_entries_and_the_abi_stays():
    import ctypes as C
    from sgdm_amd import _lib as L
    txt = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    for name, nargs, i64_at in (("sgd_loss_fwd", 14, 10), ("sgd_loss_bwd", 15, 12)):
        res, args = L.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == nargs and args[i64_at] is C.c_int64
        proto = re.search(r"int %s\(([^;]*)\);" % name, txt).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == nargs
    assert L.SIGNATURES["sgd_loss_bwd"][1][8] is C.c_float and L.SIGNATURES["sgd_loss_bwd"][1][7] is L.dvp
    assert "sgd_mse_loss" in L.SIGNATURES                       # stays as it is
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "loss.hip" in b._sources() and b.FILE_FLAGS["loss.hip"] == ["-ffp-contract=off"]
    from sgdm_amd.losses import _LOSS_KIND, _LOSS_PAR
    assert _LOSS_PAR == dict(eps=0, x0=1, v=2) and _LOSS_KIND == dict(l2=0, l1=1, huber=2)
