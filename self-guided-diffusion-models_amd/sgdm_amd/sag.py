"""Self-attention guidance (Hong et al., ICCV 2023; sampling kwargs sag_scale / sag_layer / sag_threshold / sag_blur_sigma)
restated in torch: what the two launches of csrc/sag.hip compute, in the kernels' operation order and in the dtype of the
input -- fp32 reproduces sgd_sag_degrade product by product, float64 is the reference of the tolerance tests.  Pure torch, any
device; the sampling path never calls these (a missing kernel is an error, not a fall-back).  The reference project has no
such guidance."""
import math

import torch

from .sampling_plan import SAG_TAPS

PAR_ID = dict(eps=0, x0=1, v=2)                     # the ``par`` argument of sgd_sag_degrade


def gaussian_taps(sigma, taps=SAG_TAPS):
    """g[k] = exp(-k^2 / 2 sigma^2) / sum, k = -(taps // 2) .. taps // 2, in float64 (``.float()`` rounds it once: the DEVICE
    table sgd_sag_degrade reads)"""
    r = taps // 2
    g = [math.exp(-(k * k) / (2.0 * float(sigma) ** 2)) for k in range(-r, r + 1)]
    return torch.tensor(g, dtype=torch.float64) / math.fsum(g)


def qk_views(qkv, heads, dp, layout):
    """(q, k) as [n, T, heads, dp] views of an attention layer's qkv buffer [n, T, 3 * heads * dp]; ``layout``: the tape's
    ``qkv_layout`` = (head stride, k offset, v offset), which is all that tells the legacy order from the new one"""
    hs, ko, _ = layout
    n, T, ld = qkv.shape
    view = lambda off: qkv.as_strided((n, T, heads, dp), (T * ld, ld, hs, 1), qkv.storage_offset() + off)
    return view(0), view(ko)


def sag_mass_torch(q, k, lse, scale):
    """mass[b, j] = (1 / heads) sum_h sum_i exp(scale <q[b,i,h,:], k[b,j,h,:]> - lse[b,h,i]): the attention each key receives,
    mean over heads.  q [b, tq, heads, d], k [b, tk, heads, d], lse [b, heads, tq] -> [b, tk]"""
    logits = torch.einsum("bihc,bjhc->bhij", q, k) * scale
    return torch.exp(logits - lse.unsqueeze(-1)).sum(2).sum(1) / q.shape[2]


def _reflect(i, n):
    """torch's 'reflect' on an index tensor, -n < i < 2n - 1"""
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))


def sag_mask(mass, mh, mw, h, w, thr):
    """[b, 1, h, w] bool: the fp32 mass upsampled by nearest neighbour with integer arithmetic, compared in fp32"""
    ys = (torch.arange(h, device=mass.device) * mh) // h
    xs = (torch.arange(w, device=mass.device) * mw) // w
    m = mass.float().reshape(-1, mh, mw)[:, ys][:, :, xs]
    return (m > torch.tensor(float(thr), dtype=torch.float32, device=mass.device)).unsqueeze(1)


def sag_blur_torch(x0, taps):
    """the separable blur of sgd_sag_degrade over the last two dims: horizontal pass, then vertical, reflected borders, taps
    accumulated in ascending k, every product rounded before it is added"""
    r = taps.numel() // 2
    h, w = x0.shape[-2:]
    cols, rows = torch.arange(w, device=x0.device), torch.arange(h, device=x0.device)
    hp = None
    for j in range(taps.numel()):
        term = taps[j] * x0[..., _reflect(cols + (j - r), w)]
        hp = term if hp is None else hp + term
    bl = None
    for j in range(taps.numel()):
        term = taps[j] * hp[..., _reflect(rows + (j - r), h), :]
        bl = term if bl is None else bl + term
    return bl


def sag_split_torch(x, o, par, a, s):
    """(x0, eps) of the network output ``o`` at the image ``x`` (same shape), a = sqrt(ac), s = sqrt(1 - ac) broadcastable"""
    if par == "eps":
        return (x - s * o) / a, o
    if par == "x0":
        return o, (x - a * o) / s
    if par == "v":
        return a * x - s * o, a * o + s * x
    raise NotImplementedError(f"parameterization '{par}'")


def sag_degrade_torch(x, out_nhwc, par, t, sa_tab, s1_tab, mass, mh, mw, thr, taps):
    """sgd_sag_degrade: x [b, c, h, w], out_nhwc [b, h*w, >= c] (channels [0, c) are read), t long [b], the two fp32 schedule
    tables, mass [b, mh*mw] (thresholded in fp32 whatever the working dtype), taps [9].  Works in ``x.dtype``."""
    b, c, h, w = x.shape
    dt = x.dtype
    a, s = (tab[t].to(dt).view(b, 1, 1, 1) for tab in (sa_tab, s1_tab))
    o = out_nhwc.reshape(b, h, w, -1)[..., :c].permute(0, 3, 1, 2).to(dt)
    x0, e = sag_split_torch(x, o, par, a, s)
    x0d = torch.where(sag_mask(mass, mh, mw, h, w, thr), sag_blur_torch(x0, taps.to(dt)), x0)
    return a * x0d + s * e
