"""The PNDM sampler's host side (sgdm_amd/diffusion.py: PNDM_Sampler) against what the reference's PNDMScheduler recorded
(tests/golden/pndm.npz, make_golden_pndm.py): its own alphas_cumprod table, the warm-up / multistep time lists and the
per-evaluation transfer scalars.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, load_npz

NS = (3, 4, 10, 13, 25, 50, 250, 1000)


def _sampler():
    import bench
    from sgdm_amd.diffusion import LatentDiffusion
    return LatentDiffusion(device="cpu", **bench.MODEL_PARAMS).sampler_list["pndm"]


def test_pndm_is_registered_and_built_without_the_gpu():
    code = ("import bench, torch\n"
            "from sgdm_amd.diffusion import LatentDiffusion, PNDM_Sampler\n"
            "d = LatentDiffusion(device='cpu', **bench.MODEL_PARAMS)\n"
            "assert isinstance(d.sampler_list['pndm'], PNDM_Sampler)\n"
            "assert not torch.cuda.is_initialized()\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, PKG]))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr


def test_alphas_cumprod_equals_the_reference_scheduler():
    v = load_npz("pndm.npz")
    ac = _sampler().alphas_cumprod
    assert ac.dtype == torch.float32 and tuple(ac.shape) == (1001,)
    assert np.array_equal(ac.numpy(), v["alphas_cumprod"])
    assert float(ac[-1]) == 0.0


@pytest.mark.parametrize("n", NS)
def test_time_lists_equal_the_reference(n):
    v = load_npz("pndm.npz")
    warmup, plms = _sampler().time_steps(n)
    assert warmup == v[f"n{n}.warmup"].tolist()
    assert plms == v[f"n{n}.plms"].tolist()
    times, tab = _sampler().plan(n)
    assert times == warmup + plms and tuple(tab.shape) == (len(times), 8) and tab.dtype == torch.int32


@pytest.mark.parametrize("n", [1, 2, 1001])
def test_step_counts_the_reference_cannot_run_raise(n):
    """the reference fails with ValueError for fewer than four inference times (n = 1, 2: numpy broadcast in
    get_warmup_time_steps) and for n > 1000 (range() step 0).  n = 3 still yields four times (step 333) and runs there."""
    with pytest.raises(ValueError):
        _sampler().time_steps(n)


@pytest.mark.parametrize("n", [10, 13])
def test_update_table_restated_in_torch_reproduces_the_reference_bit_for_bit(n):
    """the sgd_pndm_row table drives the kernel's update; applied here with torch fp32 CPU ops in the kernel's order to the
    reference's recorded residuals, it must reproduce every recorded UNet input and the final image exactly"""
    v = load_npz("pndm.npz")
    times, tab = _sampler().plan(n)
    assert times == v[f"pndm{n}.t"].tolist()
    coef = tab[:, :3].view(torch.float32)
    k16, k13, k124 = (torch.tensor(np.float32(1 / q)) for q in (6, 3, 24))
    x = torch.from_numpy(v[f"pndm{n}.x_T"])
    eps, x_in = torch.from_numpy(v[f"pndm{n}.eps"]), torch.from_numpy(v[f"pndm{n}.x_in"])
    ring, acc, base = [None] * 3, None, None
    for k in range(len(times)):
        assert torch.equal(x, x_in[k]), k
        e, (d, c1, c2) = eps[k], coef[k]
        phase, s1, s2, s3 = tab[k, 4:].tolist()
        if phase == 0:
            acc, base, ring[s1], src, r = k16 * e, x, e, x, e
        elif phase == 1:
            acc, src, r = acc + k13 * e, base, e
        elif phase == 2:
            src, r = base, acc + k16 * e
        else:
            src, r = x, k124 * (55 * e - 59 * ring[s1] + 37 * ring[s2] - 9 * ring[s3])
            ring[s3] = e
        x = src + d * (c1 * src - c2 * r)
    assert torch.equal(x, torch.from_numpy(v[f"pndm{n}.final"]))


@pytest.mark.parametrize("n", [10, 13, 50, 250])
def test_transfer_scalars_are_correctly_rounded_fp32(n):
    """every op of the reference's transfer expression rounded once to fp32 (evaluated here in float64 and rounded after each
    op, which is exact rounding for +, -, *, / and sqrt of fp32 operands): the table must not depend on the host's libraries"""
    s = _sampler()
    warmup, plms = s.time_steps(n)
    times, tab = s.plan(n)
    ac = s.alphas_cumprod.numpy().astype(np.float64)
    f = lambda v: float(np.float32(v))
    coef = tab[:, :3].view(torch.float32).numpy()
    prev_next = [(warmup[j // 4 * 4], warmup[min(j + 1, 11)]) for j in range(12)] + \
                [(t, plms[min(k + 1, len(plms) - 1)]) for k, t in enumerate(plms)]
    for k, (tp, tn) in enumerate(prev_next):
        at, an = ac[tp + 1], ac[tn + 1]
        sa, sn = f(np.sqrt(at)), f(np.sqrt(an))
        c1 = f(1.0 / f(sa * f(sa + sn)))
        c2 = f(1.0 / f(sa * f(f(np.sqrt(f(f(1.0 - an) * at))) + f(np.sqrt(f(f(1.0 - at) * an))))))
        assert (float(coef[k, 0]), float(coef[k, 1]), float(coef[k, 2])) == (f(an - at), c1, c2), k
