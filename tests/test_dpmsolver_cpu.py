"""The DPM-Solver++(2M) sampler's host side (sgdm_amd/diffusion.py: DPMSolverSampler.plan).  The reference has no such
sampler, so the expected values are the method's formulas restated here in float64, independently of the code under test:

    lam(v) = log(v / (1 - v)) / 2;  per visited table index ts[i]: at = a[ts[i]], ap = a[ts[i-1]] (a[0] for i = 0)
    x0 = (x - sqrt(1-at) e) / sqrt(at);  D = cc x0 + cp x0_prev;  x_next = A x + B D
    A = sqrt((1-ap)/(1-at)), B = sqrt(ap) - A sqrt(at), h = lam(ap) - lam(at), r = h_prev / h, cc = 1 + 1/(2r), cp = -1/(2r)

No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT

T = 1000
SPACINGS = ("logsnr", "uniform", "quad")


def _diffusion():
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **bench.MODEL_PARAMS)


def _sk(d, S, **kw):
    return dict(dict(num_timesteps=S, ddim_eta=0.0, clip_denoised=True, dtp=1, temperature=1.0, noise_dropout=0,
                     log_num_per_prog=10, vis=None, alphas_cumprod=d.sampler.alphas_cumprod), **kw)


def _lam(v):
    return 0.5 * np.log(v / (1.0 - v))


def _times(a, S, kind):
    """the issue's three spacings, restated"""
    from sgdm_amd.diffusion import make_ddim_timesteps
    if kind == "uniform":
        return np.asarray(make_ddim_timesteps("uniform", S, T))
    if kind == "quad":
        return np.unique(make_ddim_timesteps("quad", S, T))
    targets = np.linspace(_lam(a[T - 1]), _lam(a[1]), S)
    grid = _lam(a[1:T])
    return np.unique([1 + int(np.argmin(np.abs(grid - v))) for v in targets])


def _expected(a, ts, order, lof):
    """[n, 6] float64: s1ma, rsa, A, B, cc, cp, row by row with scalar math"""
    n = len(ts)
    rows, h_prev = [None] * n, None
    for k, i in enumerate(reversed(range(n))):
        at, ap = a[ts[i]], (a[ts[i - 1]] if i > 0 else a[0])
        A = np.sqrt((1 - ap) / (1 - at))
        B = np.sqrt(ap) - A * np.sqrt(at)
        h = _lam(ap) - _lam(at)
        if k == 0 or order == 1 or (lof and i == 0):
            cc, cp = 1.0, 0.0
        else:
            r = h_prev / h
            cc, cp = 1 + 1 / (2 * r), -1 / (2 * r)
        rows[i] = (np.sqrt(1 - at), 1 / np.sqrt(at), A, B, cc, cp)
        h_prev = h
    return np.array(rows, dtype=np.float64)


def _ulps(got32, want64):
    """|got - fp32(want)| in units of the spacing of fp32 at want"""
    want32 = want64.astype(np.float32)
    return np.abs(got32.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def test_dpmsolver_is_registered_and_planned_without_the_gpu():
    code = ("import bench, torch\n"
            "from sgdm_amd.diffusion import LatentDiffusion, DPMSolverSampler\n"
            "d = LatentDiffusion(device='cpu', **bench.MODEL_PARAMS)\n"
            "s = d.sampler_list['dpmsolver']\n"
            "assert isinstance(s, DPMSolverSampler)\n"
            "ts, tab = s.plan(dict(num_timesteps=20, alphas_cumprod=d.sampler.alphas_cumprod))\n"
            "assert tab.dtype == torch.float32 and tuple(tab.shape) == (len(ts), 8) and tab.device.type == 'cpu'\n"
            "assert 2 <= len(ts) <= 20\n"
            "assert not torch.cuda.is_initialized()\n"
            "import sgdm_amd._lib as L\n"
            "assert L._lib is None\n")                 # planning does not load the library either
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]), CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("S", [4, 10, 20, 50])
def test_table_equals_the_formulas_in_float64(S, kind, order):
    d = _diffusion()
    s = d.sampler_list["dpmsolver"]
    a = d.sampler.alphas_cumprod.double().numpy()
    want_ts = _times(a, S, kind)
    for lof in (None, True, False):
        ts, tab = s.plan(_sk(d, S, dpm_spacing=kind, dpm_order=order, dpm_lower_order_final=lof))
        assert np.array_equal(np.asarray(ts), want_ts)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == (len(ts), 8)
        eff = len(ts) < 15 if lof is None else lof
        want = _expected(a, want_ts, order, eff)
        got = tab.numpy()
        # <= 1 ulp: two float64 evaluations of log may differ in the last place, which can move an fp32 rounding boundary
        u = _ulps(got[:, :6], want)
        assert u.max() <= 1.0, (u.max(), np.unravel_index(u.argmax(), u.shape))
        assert np.all(got[:, 6:] == 0)
        n = len(ts)
        first = [n - 1] + ([0] if eff else []) if order == 2 else list(range(n))
        for i in range(n):
            if i in first:
                assert got[i, 4] == 1.0 and got[i, 5] == 0.0, (i, got[i])
            else:
                assert got[i, 5] < 0.0 and got[i, 4] > 1.0, (i, got[i])       # a true second-order row
        # cc and cp are rounded separately (half an ulp each, cc the larger): their sum is 1 to one ulp of cc
        s64 = got[:, 4].astype(np.float64) + got[:, 5].astype(np.float64)
        assert np.all(np.abs(s64 - 1.0) <= np.spacing(got[:, 4]).astype(np.float64))
    # the default is order 2 on the log-SNR spacing
    ts_d, tab_d = s.plan(_sk(d, S))
    ts_e, tab_e = s.plan(_sk(d, S, dpm_spacing="logsnr", dpm_order=2, dpm_lower_order_final=None))
    assert np.array_equal(ts_d, ts_e) and torch.equal(tab_d, tab_e)


@pytest.mark.parametrize("S", [10, 20, 50, 250])
def test_first_order_uniform_rows_are_ddims_coefficients(S):
    """x_next = A x + B x0 with x0 = (x - sqrt(1-at) e) / sqrt(at) is DDIM's sqrt(ap) x0 + sqrt(1-ap) e (eta = 0) when
    B + A sqrt(at) == sqrt(ap) and A sqrt(1-at) == sqrt(1-ap), DDIM's own tables on the right-hand sides"""
    from sgdm_amd.diffusion import DDIMSampler
    d = _diffusion()
    sk = _sk(d, S, dpm_spacing="uniform", dpm_order=1)
    ts, tab = d.sampler_list["dpmsolver"].plan(sk)
    ddim = DDIMSampler(ddpm_num_timesteps=T, device="cpu", sampler_type="ddim")
    ddim.make_schedule(sk)
    assert np.array_equal(np.asarray(ts), ddim.ddim_timesteps)
    at = np.asarray(ddim.ddim_alphas, dtype=np.float64)
    ap = np.asarray(ddim.ddim_alphas_prev, dtype=np.float64)
    s1ma = np.asarray(ddim.ddim_sqrt_one_minus_alphas, dtype=np.float64)
    t = tab.double().numpy()
    A, B = t[:, 2], t[:, 3]
    assert np.all(t[:, 4] == 1) and np.all(t[:, 5] == 0)
    np.testing.assert_allclose(B + A * np.sqrt(at), np.sqrt(ap), rtol=1e-6, atol=0)
    np.testing.assert_allclose(A * s1ma, np.sqrt(1 - ap), rtol=1e-6, atol=0)
    np.testing.assert_allclose(t[:, 0], s1ma, rtol=1e-6, atol=0)
    np.testing.assert_allclose(t[:, 1] * np.sqrt(at), 1.0, rtol=1e-6, atol=0)


S2 = 0.25
X_T = np.random.default_rng(0).standard_normal(4096)


def _toy_error(d, S, kind, order):
    """rel-L2 error of the TABLE, applied in numpy float64 to the exact noise prediction of N(0, S2) data, against the
    closed-form probability-flow solution"""
    a = d.sampler.alphas_cumprod.double().numpy()
    ts, tab = d.sampler_list["dpmsolver"].plan(_sk(d, S, dpm_spacing=kind, dpm_order=order))
    t = tab.double().numpy()
    x, x0p = X_T.copy(), np.zeros_like(X_T)
    for i in reversed(range(len(ts))):
        at = a[ts[i]]
        e = np.sqrt(1 - at) * x / (at * S2 + 1 - at)
        s1ma, rsa, A, B, cc, cp = t[i, :6]
        x0 = (x - s1ma * e) * rsa
        x = A * x + B * (cc * x0 + cp * x0p)
        x0p = x0
    exact = X_T * np.sqrt((a[0] * S2 + 1 - a[0]) / (a[ts[-1]] * S2 + 1 - a[ts[-1]]))
    return float(np.sqrt(((x - exact) ** 2).sum() / (exact ** 2).sum()))


@pytest.mark.parametrize("kind", ["logsnr", "quad"])
@pytest.mark.parametrize("S", [10, 15, 20, 50])
def test_second_order_beats_first_order_by_four(S, kind):
    d = _diffusion()
    e1, e2 = _toy_error(d, S, kind, 1), _toy_error(d, S, kind, 2)
    print(f"toy {kind} S={S}: order 1 {e1:.3e}, order 2 {e2:.3e}, ratio {e1 / e2:.1f}")
    assert e2 <= e1 / 4


def test_second_order_beats_first_order_by_two_on_uniform_50():
    d = _diffusion()
    e1, e2 = _toy_error(d, 50, "uniform", 1), _toy_error(d, 50, "uniform", 2)
    print(f"toy uniform S=50: order 1 {e1:.3e}, order 2 {e2:.3e}, ratio {e1 / e2:.1f}")
    assert e2 <= e1 / 2


@pytest.mark.parametrize("kind", SPACINGS)
def test_second_order_error_falls_with_the_step_count(kind):
    """second order gives 4x per halving of the step; at least 2.5x is asked"""
    d = _diffusion()
    e25, e50 = _toy_error(d, 25, kind, 2), _toy_error(d, 50, kind, 2)
    print(f"toy {kind}: order 2 at S=25 {e25:.3e}, S=50 {e50:.3e}, drop {e25 / e50:.2f}")
    assert e25 / e50 >= 2.5


@pytest.mark.parametrize("bad", [dict(dpm_order=3), dict(dpm_order=0), dict(dpm_spacing="cosine"), dict(num_timesteps=1),
                                 dict(num_timesteps=1, dpm_spacing="uniform"), dict(num_timesteps=1, dpm_spacing="quad")])
def test_plan_refuses_what_it_cannot_do(bad):
    d = _diffusion()
    with pytest.raises(ValueError):
        d.sampler_list["dpmsolver"].plan(_sk(d, 20, **bad))


def test_dynamic_thresholding_is_refused_before_anything_is_launched():
    d = _diffusion()
    called = []
    with pytest.raises(ValueError):
        d.sampler_list["dpmsolver"].sample(shape=(2, 3, 16, 16), sampling_kwargs=_sk(d, 20, dtp=0.9),
                                           denoise_sample_fn=lambda *a, **k: called.append(1), denoise_sample_fn_kwargs={})
    assert not called
