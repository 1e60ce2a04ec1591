"""Nearest-x2-upsample 3x3 convs as four 2x2 sub-pixel convs at the input resolution (SGD_RS_UP2_SUBPIXEL).

CPU: the identity itself in float64 (16 summed kernels at low resolution == nearest-up + 3x3 conv), and the shared rule
sgd_igemm_subpixel_ok.  GPU: the sub-pixel launch against float64 torch and against the direct SGD_RS_UP2 launch at the
production shapes (UNet batch 80) and at small batches, its parity-aware epilogue statistics, bit-repeatability, the batched
pack job, and one whole C2 evaluation with the path on and off against the oracle.
"""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel

# R(a)[r]: the 3x3 rows (ky = dy + 1) that kernel row r of output parity a sums
ROWS = {0: ([0], [1, 2]), 1: ([0, 1], [2])}


def subpixel_kernels(w):
    """[cout, cin, 3, 3] -> V[a][b] = [cout, cin, 2, 2]"""
    V = [[None, None], [None, None]]
    for a in (0, 1):
        for b in (0, 1):
            k = torch.zeros(w.shape[0], w.shape[1], 2, 2, dtype=w.dtype)
            for r in (0, 1):
                for s in (0, 1):
                    k[:, :, r, s] = w[:, :, ROWS[a][r]][:, :, :, ROWS[b][s]].sum((2, 3))
            V[a][b] = k
    return V


def subpixel_conv(h, w, bias=None):
    """y[2i+a, 2j+b] = sum_{r,s} V[a][b][r][s] h[i+a-1+r, j+b-1+s] (zero outside h)"""
    n, _, H, W = h.shape
    V = subpixel_kernels(w)
    hp = F.pad(h, (1, 1, 1, 1))
    y = torch.empty(n, w.shape[0], 2 * H, 2 * W, dtype=h.dtype)
    for a in (0, 1):
        for b in (0, 1):
            y[:, :, a::2, b::2] = F.conv2d(hp[:, :, a:a + H + 1, b:b + W + 1], V[a][b], bias)
    return y


@pytest.mark.parametrize("shape", [(1, 3, 2, 2, 5), (3, 4, 2, 4, 2), (5, 2, 8, 8, 3), (2, 6, 4, 16, 4), (1, 1, 1, 1, 1)])
def test_subpixel_identity_float64(shape):
    n, cin, H, W, cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    h = torch.randn(n, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), w, b, padding=1)
    got = subpixel_conv(h, w, b)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _args(n, hi, wi, c0, cout, prec, c1=0, rs=2, stats=False, tune=0):
    L, _ = _lib()
    a = L.IgemmArgs()
    a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride, a.resample = L.MODE_CONV3, n, hi, wi, 2 * hi, 2 * wi, 1, rs
    a.c0, a.c1, a.cout, a.y_ld, a.prec, a.tune = c0, c1, cout, cout, prec, tune
    a.stats = 1 if stats else 0
    return a


def test_subpixel_rule():
    """sgd_igemm_subpixel_ok: the production shapes qualify in both split modes; never in f32, with the tune bit, for
    non-16-byte channel counts, for 32-column tiles, or for statistics of two images per tile"""
    L, lib = _lib()
    ok = lambda *p, **k: lib.sgd_igemm_subpixel_ok(C.byref(_args(*p, **k)))
    for prec in (L.PREC_F16X3, L.PREC_BF16X3):
        assert ok(80, 16, 16, 512, 512, prec, stats=True) == 1
        assert ok(80, 32, 32, 256, 256, prec, stats=True) == 1
        assert ok(80, 16, 16, 512, 512, prec, rs=L.RS_UP2_SUBPIXEL) == 1
        assert ok(80, 16, 16, 512, 512, prec, tune=L.TUNE_NO_SUBPIXEL) == 0
        assert ok(80, 16, 16, 510, 512, prec) == 0                   # channels not a multiple of 4
        assert ok(80, 16, 16, 512, 96, prec) == 0                    # 32-column tile (cout % 128)
        assert ok(1, 8, 8, 256, 256, prec) == 0                      # small launch: the 32-column tile
        assert ok(80, 8, 8, 256, 256, prec, stats=True) == 0         # 64-pixel input map: two images per tile
        assert ok(80, 8, 8, 256, 256, prec, stats=False) == 1
        assert ok(80, 16, 16, 512, 512, prec, rs=L.RS_NONE) == 0
    assert ok(80, 16, 16, 512, 512, L.PREC_F32, stats=True) == 0
    # the parity-aware statistics slots: [parity][input-resolution tile], as many as the direct launch's
    a = _args(80, 16, 16, 512, 512, L.PREC_F16X3, rs=L.RS_UP2_SUBPIXEL)
    d = _args(80, 16, 16, 512, 512, L.PREC_F16X3)
    a.cout_p = d.cout_p = 512
    assert lib.sgd_igemm_stats_parts(C.byref(a)) == 4 * 2 == lib.sgd_igemm_stats_parts(C.byref(d))
    assert lib.sgd_packed_weight_subpixel_bytes(512, 512, L.PREC_F16X3) == 16 * 512 * 512 * 4


# ------------------------------------------------------------------------------------------------------------------- GPU
PRECS = [("f16x3", 2e-5), ("bf16x3", 1e-4)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _pack(w, prec, sub):
    """scaled pack of the direct (sub=False) or the sub-pixel weights; returns (buf, cin_p, cout_p, scale_inv, amax)"""
    L, lib = _lib()
    cout, cin = w.shape[0], w.shape[1]
    nb = lib.sgd_packed_weight_subpixel_bytes(cout, cin, prec) if sub else lib.sgd_packed_weight_bytes(cout, cin, 3, prec)
    buf = torch.empty(nb // 4, device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    sinv = torch.ones(1, device="cuda")
    cp, op = C.c_int32(), C.c_int32()
    if sub:
        L.check(lib.sgd_weight_amax_subpixel(_p(w), cout, cin, _p(amax), _stream()), "amax_subpixel")
        L.check(lib.sgd_pack_weight_subpixel_scaled(_p(w), _p(buf), cout, cin, prec, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                                    _stream()), "pack_subpixel")
    else:
        L.check(lib.sgd_weight_amax(_p(w), w.numel(), _p(amax), _stream()), "amax")
        L.check(lib.sgd_pack_weight_scaled(_p(w), _p(buf), cout, cin, 3, prec, 0, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                           _stream()), "pack")
    return buf, cp.value, op.value, sinv, amax


def _launch(x, w, bias, prec, sub, pa=None, pb=None, stats=False, packed=None, tune=0):
    """x: NHWC cuda at the INPUT resolution; returns (y NHWC at 2x, reduced statistics [n, cout, 2] or None)"""
    L, lib = _lib()
    n, hi, wi, c0 = x.shape
    cout = w.shape[0]
    buf, cp, op, sinv, _ = packed if packed is not None else _pack(w, prec, sub)
    a = _args(n, hi, wi, c0, cout, prec, rs=L.RS_UP2_SUBPIXEL if sub else L.RS_UP2, tune=tune)
    a.x0, a.w, a.cin_p, a.cout_p, a.w_scale_inv = x.data_ptr(), buf.data_ptr(), cp, op, sinv.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else 0
    if pa is not None:
        a.pro, a.pro_silu, a.pa, a.pb = L.PRO_AFFINE_NC, 1, pa.data_ptr(), pb.data_ptr()
    y = torch.full((n, 2 * hi, 2 * wi, cout), float("nan"), device="cuda")
    a.y = y.data_ptr()
    part = None
    a.stats = 0
    if stats:
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts > 0
        part = torch.full((n, parts, 2, cout), float("nan"), device="cuda")
        a.stats = part.data_ptr()
    L.check(lib.sgd_igemm(C.byref(a), _stream()), "igemm")
    sums = None
    if stats:
        sums = torch.zeros(n, cout, 2, device="cuda")
        L.check(lib.sgd_stats_reduce(_p(part), n, parts, cout, _p(sums), cout, 0, _stream()), "reduce")
    torch.cuda.synchronize()
    return y, sums


def _reference(x, w, bias, pa, pb, idx):
    """float64 nearest-up + 3x3 conv of images idx (NHWC in, NHWC out), on the device"""
    h = x[idx].double().permute(0, 3, 1, 2)
    if pa is not None:
        h = F.silu(h * pa[idx].double()[:, :, None, None] + pb[idx].double()[:, :, None, None])
    y = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), w.double(), bias.double() if bias is not None else None,
                 padding=1)
    return y.permute(0, 2, 3, 1)


def _data(n, hi, c, cout, seed, prologue=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hi, hi, c, generator=g).cuda()
    w = (torch.randn(cout, c, 3, 3, generator=g) / math.sqrt(c * 9)).cuda()
    b = torch.randn(cout, generator=g).cuda()
    pa = (1.0 + 0.3 * torch.randn(n, c, generator=g)).cuda() if prologue else None
    pb = (0.3 * torch.randn(n, c, generator=g)).cuda() if prologue else None
    return x, w, b, pa, pb


SUBSET = [0, 1, 39, 40, 78, 79]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("shape", [(80, 16, 512, 512), (80, 32, 256, 256)])
def test_subpixel_resblock_up_at_unet_batch_80(shape, prec, tol):
    """output_blocks.2.2 / output_blocks.5.1 in_layers.2 of C2: GroupNorm + SiLU prologue, bias, fused statistics"""
    L, _ = _lib()
    n, hi, c, cout = shape
    x, w, b, pa, pb = _data(n, hi, c, cout, 11 + hi)
    pr = L.PREC_BY_NAME[prec]
    ys, ss = _launch(x, w, b, pr, True, pa, pb, stats=True)
    yd, sd = _launch(x, w, b, pr, False, pa, pb, stats=True)
    assert not torch.isnan(ys).any()
    assert max_rel(ys[SUBSET], _reference(x, w, b, pa, pb, SUBSET)) < tol
    assert max_rel(ys, yd) < 2 * tol
    # parity-aware statistics folded by sgd_stats_reduce: the direct path's sums, and the exact sums of the sub-pixel output
    exact = torch.stack([ys.double().sum((1, 2)), (ys.double() ** 2).sum((1, 2))], -1)
    assert max_rel(ss, exact) < 2e-6
    assert max_rel(ss, sd) < 4 * tol
    ys2, ss2 = _launch(x, w, b, pr, True, pa, pb, stats=True)
    assert torch.equal(ys, ys2) and torch.equal(ss, ss2), "two sub-pixel launches differ"


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("tile", ["bn128", "bn256"])
def test_subpixel_both_tiles(tile, prec, tol):
    """the 128-column (16x16x32) and the 128 x 256 (32x32x16) instances against float64 and against each other"""
    L, _ = _lib()
    x, w, b, pa, pb = _data(7, 16, 256, 256, 5)
    pr = L.PREC_BY_NAME[prec]
    tune = L.TUNE_BN128 if tile == "bn128" else L.TUNE_BN256
    y, _ = _launch(x, w, b, pr, True, pa, pb, tune=tune | L.TUNE_NO_SMALL)
    assert max_rel(y, _reference(x, w, b, pa, pb, list(range(7)))) < tol


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("n", [1, 3, 7])
@pytest.mark.parametrize("shape", [(16, 256, 256, True), (32, 128, 128, True), (8, 512, 512, False), (16, 256, 256, False)])
def test_subpixel_small_batches(shape, n, prec, tol):
    """ResBlock-up (GroupNorm + SiLU prologue) and plain Upsample(use_conv=True) shapes (C5: 8^2 / 16^2 inputs, no
    prologue) at batches 1, 3, 7, with the tile rule pinned to the 128-column tile so that the small launches run it too"""
    L, _ = _lib()
    hi, c, cout, pro = shape
    x, w, b, pa, pb = _data(n, hi, c, cout, 100 + n + hi, prologue=pro)
    pr = L.PREC_BY_NAME[prec]
    y, _ = _launch(x, w, b, pr, True, pa, pb, tune=L.TUNE_NO_SMALL)
    assert max_rel(y, _reference(x, w, b, pa, pb, list(range(n)))) < tol
    yd, _ = _launch(x, w, b, pr, False, pa, pb, tune=L.TUNE_NO_SMALL)
    assert max_rel(y, yd) < 2 * tol


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
def test_subpixel_batched_pack_job_equals_single_pack(prec):
    """sgd_pack_weights_batched with a SGD_PACK_SUBPIXEL job == sgd_weight_amax_subpixel + sgd_pack_weight_subpixel_scaled"""
    L, lib = _lib()
    pr = L.PREC_BY_NAME[prec]
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(256, 128, 3, 3, generator=g) * 1e-3).cuda()
    buf, cp, op, sinv, amax = _pack(w, pr, True)
    ab, pb, cp2, op2 = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    L.check(lib.sgd_pack_job_blocks(256, 128, 3, pr, L.PACK_SUBPIXEL, C.byref(ab), C.byref(pb), C.byref(cp2), C.byref(op2)),
            "blocks")
    assert (cp2.value, op2.value) == (cp, op)
    buf2 = torch.full_like(buf, float("nan"))
    amax2 = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    sinv2 = torch.zeros(1, device="cuda")
    job = L.PackJob(src=w.data_ptr(), dst=buf2.data_ptr(), amax_bits=amax2.data_ptr(), scale_inv=sinv2.data_ptr(), cout=256,
                    cin=128, ksize=3, transpose=L.PACK_SUBPIXEL, own_amax=1)
    jobs = torch.frombuffer(bytearray(C.string_at(C.addressof(job), C.sizeof(job))), dtype=torch.uint8).cuda()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    # (the block tables stay referenced until the launches have run)
    a_job, a_first, p_job, p_first = i32([0] * ab.value), i32([0, ab.value]), i32([0] * pb.value), i32([0, pb.value])
    L.check(lib.sgd_pack_weights_batched(_p(jobs), 1, _p(a_job), _p(a_first), ab.value, _p(p_job), _p(p_first), pb.value, pr,
                                         _stream()), "batched")
    torch.cuda.synchronize()
    assert torch.equal(amax, amax2) and torch.equal(sinv, sinv2)
    assert torch.equal(buf.view(torch.int32), buf2.view(torch.int32))
    # the scale is that of max |V|, not max |W|
    V = subpixel_kernels(w.cpu().double())
    vmax = max(float(V[a][b].abs().max()) for a in (0, 1) for b in (0, 1))
    assert float(amax.view(torch.float32)) == pytest.approx(vmax, rel=1e-6)


@pytest.mark.gpu
def test_c2_evaluation_subpixel_on_and_off_vs_oracle():
    """one CFG evaluation of C2 at UNet batch 80 in f16x3 with the sub-pixel launches (the default) and without them
    (SGDM_SUBPIXEL=0), both against the oracle under the full-size tolerance; exact f32 never takes the path"""
    import test_hip_fullsize as FS
    from oracle import unet_ref as U
    wl, m, sd, data = FS._bench_model("c2", "f16x3")
    B, S = wl["batch"], wl["image"]
    cfg = FS._oracle_cfg(wl)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, 3, S, S, generator=g)
    t = torch.full((B,), 437, dtype=torch.long)
    with torch.no_grad():
        ref = U.forward_with_cond_scale(cfg, sd, x, t, 2.0, data["cond"], data.get("layout"))
    got = {}
    old = os.environ.get("SGDM_SUBPIXEL")
    try:
        for on in ("1", "0"):
            os.environ["SGDM_SUBPIXEL"] = on
            m._engines.clear()
            m.hip_precision = "f16x3"
            with torch.no_grad():
                got[on] = m.forward_with_cond_scale(x.cuda(), t.cuda(), cond=data["cond"].cuda(), cond_scale=2.0).cpu()
            eng = next(iter(m._engines.values()))
            nsub = sum(1 for pk in eng.packed if getattr(pk, "subpixel", False))
            assert (nsub >= 2) if on == "1" else nsub == 0, nsub
            assert max_rel(got[on], ref) < 5e-5, (on, max_rel(got[on], ref))
        os.environ["SGDM_SUBPIXEL"] = "1"
        m._engines.clear()
        m.hip_precision = "f32"
        with torch.no_grad():
            m.forward_with_cond_scale(x.cuda(), t.cuda(), cond=data["cond"].cuda(), cond_scale=2.0)
        eng = next(iter(m._engines.values()))
        assert not any(getattr(pk, "subpixel", False) for pk in eng.packed)
    finally:
        if old is None:
            os.environ.pop("SGDM_SUBPIXEL", None)
        else:
            os.environ["SGDM_SUBPIXEL"] = old
