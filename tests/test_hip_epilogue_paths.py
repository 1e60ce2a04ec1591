"""Every branch of the conv kernel's tile epilogue (csrc/igemm.hip: IgemmBlock::epilogue) at the smallest shapes that reach it,
through the C ABI, against a float64 torch conv / linear on the CPU.  GPU only.

Branches: residual none / same row / 2x2 average of a map at twice the resolution / nearest pixel of a map at half the
resolution, each with and without the fused GroupNorm statistics; two images per 128-row tile with the last tile half
masked; the 32-column instance with column quads beyond cout, and the scalar path (cout % 4 != 0); flat launches with masked
rows on the 32-, 128- and 256-column tile and the row-remapped output; capped grids with a workspace, one of which the balanced
tail cuts along K so that the finisher's epilogue adds the producers' slabs; the sub-pixel and the fused-aux instance.

Bounds.  Outputs: the per-mode bounds of the igemm kernel tests (test_hip_kernels.PRECS) on conftest.max_rel and
conftest.rel_l2.  Statistics slots, summed over a tile's slots, against S1 = sum y and S2 = sum y^2 of the float64 reference
over the P pixels of an image: |y - ref| <= tol * max|ref| per element gives |dS1| <= P * tol * max|ref| and
|dS2| <= P * tol * (2 + tol) * max|ref|^2; the kernel's own fp32 summation (a lane's <= 16 rows, then a 4..5-level
lane tree: < 32 roundings, each <= 2^-24 of the running sum, itself <= P * max) adds 32 * 2^-24 < 2e-6 of the same scales.
So dS1 / (P max|ref|) < tol + 2e-6 and dS2 / (P max|ref|^2) < 2.1 * tol + 2e-6.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_l2
from test_hip_kernels import PRECS              # (mode, bound) of the igemm kernel tests: f32 2e-6, f16x3 2e-5, bf16x3 1e-4

pytestmark = pytest.mark.gpu

D = torch.float64


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return C.c_void_p(t.data_ptr())


def _pack(w, ks, prec, sub=False):
    """scaled pack (one power-of-two scale per tensor, as the engine packs): (buf, cin_p, cout_p, scale_inv)"""
    L, lib = _lib()
    cout, cin = w.shape[0], w.shape[1]
    nb = lib.sgd_packed_weight_subpixel_bytes(cout, cin, prec) if sub else lib.sgd_packed_weight_bytes(cout, cin, ks, prec)
    buf = torch.empty(nb // 4, device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    sinv = torch.ones(1, device="cuda")
    cp, op = C.c_int32(), C.c_int32()
    if sub:
        L.check(lib.sgd_weight_amax_subpixel(_p(w), cout, cin, _p(amax), _st()), "amax")
        L.check(lib.sgd_pack_weight_subpixel_scaled(_p(w), _p(buf), cout, cin, prec, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                                    _st()), "pack")
    else:
        L.check(lib.sgd_weight_amax(_p(w), w.numel(), _p(amax), _st()), "amax")
        L.check(lib.sgd_pack_weight_scaled(_p(w), _p(buf), cout, cin, ks, prec, 0, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                           _st()), "pack")
    return buf, cp.value, op.value, sinv


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


_WORK = {}


def _work():
    L, lib = _lib()
    if "w" not in _WORK:
        _WORK["w"] = torch.zeros(int(lib.sgd_igemm_work_bytes()) // 4, device="cuda")
    return _WORK["w"]


def _work_healthy():
    L, lib = _lib()
    off = int(lib.sgd_igemm_work_status_offset())
    return int(_work().view(torch.int32)[off // 4]) == 0


# --------------------------------------------------------------------------------------------------------- 3x3 cases
RES_MODES = ["none", "same", "avgpool", "up"]
_CONV = {}


def conv_case(n, hw, cin, cout, res):
    """seeded inputs and the float64 reference of y = conv3x3(silu(a x + b)) + bias (+ residual), computed once per key"""
    key = (n, hw, cin, cout, res)
    if key in _CONV:
        return _CONV[key]
    g = torch.Generator().manual_seed(7 + RES_MODES.index(res) + 10 * cout + hw)
    x = torch.randn(n, cin, hw, hw, generator=g)
    pa, pb = 1 + 0.3 * torch.randn(n, cin, generator=g), 0.3 * torch.randn(n, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    b = torch.randn(cout, generator=g)
    rhw = {"none": 0, "same": hw, "avgpool": 2 * hw, "up": hw // 2}[res]
    r = torch.randn(n, cout, rhw, rhw, generator=g) if rhw else None
    ref = F.conv2d(F.silu(x.to(D) * pa.to(D)[:, :, None, None] + pb.to(D)[:, :, None, None]), w.to(D), b.to(D), padding=1)
    if res == "same":
        ref = ref + r.to(D)
    elif res == "avgpool":
        ref = ref + F.avg_pool2d(r.to(D), 2)
    elif res == "up":
        ref = ref + F.interpolate(r.to(D), scale_factor=2, mode="nearest")
    c = dict(n=n, hw=hw, cin=cin, cout=cout, res=res, ref=ref, xd=_nhwc(x).cuda(), pad=pa.cuda(), pbd=pb.cuda(), wd=w.cuda(),
             bd=b.cuda(), rd=_nhwc(r).cuda() if r is not None else None, packs={})
    _CONV[key] = c
    return c


def run_conv(c, prec_name, tune=0, stats=False, grid_cap=0, work=False):
    """-> (y NCHW cpu, statistics [n, parts, 2, cout] cpu or None)"""
    L, lib = _lib()
    prec = L.PREC_BY_NAME[prec_name]
    if prec not in c["packs"]:
        c["packs"][prec] = _pack(c["wd"], 3, prec)
    buf, cp, op, sinv = c["packs"][prec]
    n, hw, cout = c["n"], c["hw"], c["cout"]
    y = torch.full((n, hw, hw, cout), float("nan"), device="cuda")
    a = L.IgemmArgs()
    a.x0, a.c0 = c["xd"].data_ptr(), c["cin"]
    a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride = L.MODE_CONV3, n, hw, hw, hw, hw, 1
    a.pro, a.pro_silu, a.pa, a.pb = L.PRO_AFFINE_NC, 1, c["pad"].data_ptr(), c["pbd"].data_ptr()
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias = buf.data_ptr(), cp, op, sinv.data_ptr(), c["bd"].data_ptr()
    if c["rd"] is not None:
        a.res = c["rd"].data_ptr()
        a.res_mode = {"same": L.RS_NONE, "avgpool": L.RS_AVGPOOL2, "up": L.RS_UP2}[c["res"]]
    a.y, a.cout, a.y_ld, a.prec = y.data_ptr(), cout, cout, prec
    a.tune, a.grid_cap = tune, grid_cap
    if work:
        a.work, a.work_bytes = _work().data_ptr(), _work().numel() * 4
    st = None
    if stats:
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts > 0
        st = torch.full((n, parts, 2, cout), float("nan"), device="cuda")
        a.stats = st.data_ptr()
    L.check(lib.sgd_igemm(C.byref(a), _st()), "igemm")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2), (st.cpu() if st is not None else None)


def check_output(got, ref, tol, label):
    e1, e2 = max_rel(got, ref), rel_l2(got, ref)
    print(f"{label}: max-rel {e1:.3e} rel-L2 {e2:.3e} (bound {tol:.0e})")
    assert torch.isfinite(got).all()
    assert e1 < tol and e2 < tol, (label, e1, e2)


def check_stats(st, ref, tol, label):
    """st [n, parts, 2, cout] against the reference's sums over the pixels of each image (ref NCHW float64)"""
    assert torch.isfinite(st).all()
    n, cout = ref.shape[:2]
    P = ref.shape[2] * ref.shape[3]
    mx = float(ref.abs().max())
    s = st.double().sum(1)
    d1 = float((s[:, 0] - ref.sum((2, 3))).abs().max()) / (P * mx)
    d2 = float((s[:, 1] - (ref * ref).sum((2, 3))).abs().max()) / (P * mx * mx)
    print(f"{label}: statistics dS1 {d1:.3e} (bound {tol + 2e-6:.1e}) dS2 {d2:.3e} (bound {2.1 * tol + 2e-6:.1e})")
    assert d1 < tol + 2e-6 and d2 < 2.1 * tol + 2e-6, (label, d1, d2)


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("tile", [128, 32])
@pytest.mark.parametrize("res", RES_MODES)
def test_conv3x3_residual_modes(res, tile, stats, prec, tol):
    """n=3, 16x16, 32 -> 128: six 128-column tiles.  tile=128: SGD_TUNE_NO_SMALL (the launch rule alone hands so small a launch to
    the 32-column instance); tile=32: that instance (four compute waves stacked along M, four statistics slices per tile)"""
    L, lib = _lib()
    c = conv_case(3, 16, 32, 128, res)
    y, st = run_conv(c, prec, tune=L.TUNE_NO_SMALL if tile == 128 else 0, stats=stats)
    label = f"3x3 res={res} tile={tile} stats={stats} {prec}"
    check_output(y, c["ref"], tol, label)
    if stats:
        assert st.shape[1] == 2 * (1 if tile == 128 else 4)
        check_stats(st, c["ref"], tol, label)


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("res", ["none", "same"])
def test_two_images_per_tile_last_tile_half_masked(res, prec, tol):
    """n=3, 8x8, 64 -> 128: two 64-pixel images per 128-row tile, the second tile holds image 2 and 64 masked rows"""
    L, lib = _lib()
    c = conv_case(3, 8, 64, 128, res)
    y, _ = run_conv(c, prec, tune=L.TUNE_NO_SMALL)
    check_output(y, c["ref"], tol, f"8x8 two images per tile res={res} {prec}")


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("res", RES_MODES)
@pytest.mark.parametrize("cout", [36, 35])
def test_narrow_tile_clamped_quads_and_scalar_path(cout, res, prec, tol):
    """n=5, 4x4, 32 -> 36: the 32-column instance, eight 16-pixel images per tile (three masked), column quads at c >= cout in the
    second column tile; cout = 35: no 16-byte rows, the scalar path"""
    c = conv_case(5, 4, 32, cout, res)
    y, _ = run_conv(c, prec)
    check_output(y, c["ref"], tol, f"4x4 cout={cout} res={res} {prec}")


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("res", ["none", "same"])
@pytest.mark.parametrize("cap", [8, 16])
def test_split_tiles_finisher_epilogue(cap, res, stats, prec, tol):
    """n=4, 16x16, 256 -> 128 with a workspace on a capped grid: 8 tiles of 8 chunks.  On 16 blocks (two per XCD, one tile per
    XCD) the balanced tail cuts every tile along K -- asserted from the kernel's own layout functions -- so the finishers run the
    epilogue that adds the producers' slabs.  On 8 blocks (one per XCD) every block has a whole tile and, by the same functions,
    nothing is cut: that launch runs the plain epilogue on a workspace launch's full-cap grid.  Either way two runs are bit-equal
    and the plain schedule (whole tiles) gives the same values to the accumulation-order floor."""
    L, lib = _lib()
    c = conv_case(4, 16, 256, 128, res)
    out = (C.c_int32 * (4 * cap))()
    assert lib.sgd_igemm_tail_layout(8, 256 // 32, 9, cap, out) == 0
    splits = [out[4 * b] for b in range(cap)]
    print(f"grid_cap={cap}: split per block {splits}")
    assert all(sp >= 2 for sp in splits) if cap == 16 else not any(splits)
    y, st = run_conv(c, prec, tune=L.TUNE_NO_SMALL, stats=stats, grid_cap=cap, work=True)
    assert _work_healthy(), "a finisher's bounded poll expired"
    label = f"workspace grid_cap={cap} res={res} stats={stats} {prec}"
    check_output(y, c["ref"], tol, label)
    if stats:
        check_stats(st, c["ref"], tol, label)
    y2, st2 = run_conv(c, prec, tune=L.TUNE_NO_SMALL, stats=stats, grid_cap=cap, work=True)
    assert torch.equal(y, y2) and (st is None or torch.equal(st, st2))       # parts are added in a fixed order
    y3, _ = run_conv(c, prec, tune=L.TUNE_NO_SMALL | L.TUNE_PLAIN_SCHEDULE, grid_cap=cap, work=True)
    assert rel_l2(y3, y) < 2e-6


# --------------------------------------------------------------------------------------------------------- flat cases
_FLAT = {}


def flat_case(m, cin, cout, res):
    key = (m, cin, cout, res)
    if key not in _FLAT:
        g = torch.Generator().manual_seed(31 + m + cout + int(res))
        x = torch.randn(m, cin, generator=g)
        w = torch.randn(cout, cin, generator=g) / math.sqrt(cin)
        b = torch.randn(cout, generator=g)
        r = torch.randn(m, cout, generator=g) if res else None
        ref = x.to(D) @ w.to(D).t() + b.to(D)
        if res:
            ref = ref + r.to(D)
        _FLAT[key] = dict(m=m, cin=cin, cout=cout, ref=ref, xd=x.cuda(), wd=w.reshape(cout, cin, 1, 1).contiguous().cuda(), bd=b.cuda(),
                          rd=r.cuda() if res else None, packs={})
    return _FLAT[key]


def run_flat(c, prec_name, tune, remap=None, rows_per_n=0, stats=False):
    L, lib = _lib()
    prec = L.PREC_BY_NAME[prec_name]
    if prec not in c["packs"]:
        c["packs"][prec] = _pack(c["wd"], 1, prec)
    buf, cp, op, sinv = c["packs"][prec]
    m, cout = c["m"], c["cout"]
    rin, rout, roff = remap or (0, 0, 0)
    yrows = (m + rin - 1) // rin * rout if remap else m
    y = torch.full((yrows, cout), float("nan"), device="cuda")
    a = L.IgemmArgs()
    a.x0, a.c0, a.mode, a.m, a.stride, a.rows_per_n = c["xd"].data_ptr(), c["cin"], L.MODE_FLAT, m, 1, rows_per_n
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias = buf.data_ptr(), cp, op, sinv.data_ptr(), c["bd"].data_ptr()
    if c["rd"] is not None:
        a.res = c["rd"].data_ptr()
    a.y, a.cout, a.y_ld, a.prec, a.tune = y.data_ptr(), cout, cout, prec, tune
    a.orows_in, a.orows_out, a.orow_off = rin, rout, roff
    st = None
    if stats:
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts > 0
        st = torch.full((m // rows_per_n, parts, 2, cout), float("nan"), device="cuda")
        a.stats = st.data_ptr()
    L.check(lib.sgd_igemm(C.byref(a), _st()), "igemm flat")
    torch.cuda.synchronize()
    return y.cpu(), (st.cpu() if st is not None else None)


TILES = {256: "TUNE_BN256", 128: "TUNE_NO_SMALL", 32: None}


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_flat_masked_rows(tile, res, prec, tol):
    """m=200, 64 -> 256: the second 128-row tile has 56 masked rows; the 256-column tile forced by SGD_TUNE_BN256 (64 columns per
    compute wave), the 128-column tile by SGD_TUNE_NO_SMALL, and the launch rule's own choice for so small a launch (32 columns)"""
    L, lib = _lib()
    c = flat_case(200, 64, 256, res)
    y, _ = run_flat(c, prec, getattr(L, TILES[tile]) if TILES[tile] else 0)
    check_output(y, c["ref"], tol, f"flat m=200 tile={tile} res={res} {prec}")


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("tile", sorted(TILES))
def test_flat_row_remap(tile, prec, tol):
    """the same launch with its output rows re-mapped group by group (orows_in = 8 rows -> rows 2..9 of groups of 11): rows outside
    the map stay untouched"""
    L, lib = _lib()
    c = flat_case(200, 64, 256, True)
    rin, rout, roff = 8, 11, 2
    y, _ = run_flat(c, prec, getattr(L, TILES[tile]) if TILES[tile] else 0, remap=(rin, rout, roff))
    rows = (torch.arange(200) // rin) * rout + roff + torch.arange(200) % rin
    untouched = torch.ones(y.shape[0], dtype=torch.bool)
    untouched[rows] = False
    assert torch.isnan(y[untouched]).all()
    check_output(y[rows], c["ref"], tol, f"flat row remap tile={tile} {prec}")


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("tile", sorted(TILES))
def test_flat_statistics(tile, prec, tol):
    """m=256 as two images of 128 rows, 64 -> 256, residual: the statistics slots of the flat launch on every tile"""
    L, lib = _lib()
    c = flat_case(256, 64, 256, True)
    y, st = run_flat(c, prec, getattr(L, TILES[tile]) if TILES[tile] else 0, rows_per_n=128, stats=True)
    label = f"flat statistics tile={tile} {prec}"
    check_output(y, c["ref"], tol, label)
    check_stats(st, c["ref"].reshape(2, 128, 256).permute(0, 2, 1)[..., None], tol, label)


# --------------------------------------------------------------------------------------------------------- sub-pixel, fused aux
_UP = {}


def up_case():
    if not _UP:
        n, hi, cin, cout = 2, 16, 64, 128
        g = torch.Generator().manual_seed(53)
        x = torch.randn(n, cin, hi, hi, generator=g)
        pa, pb = 1 + 0.3 * torch.randn(n, cin, generator=g), 0.3 * torch.randn(n, cin, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
        b = torch.randn(cout, generator=g)
        act = F.silu(x.to(D) * pa.to(D)[:, :, None, None] + pb.to(D)[:, :, None, None])
        ref = F.conv2d(F.interpolate(act, scale_factor=2, mode="nearest"), w.to(D), b.to(D), padding=1)
        _UP.update(n=n, hi=hi, cin=cin, cout=cout, ref=ref, xd=_nhwc(x).cuda(), pad=pa.cuda(), pbd=pb.cuda(), wd=w.cuda(), bd=b.cuda())
    return _UP


def run_up(prec_name, stats):
    """-> (y NCHW cpu, statistics or None, whether the sub-pixel instance ran)"""
    L, lib = _lib()
    c = up_case()
    p = L.PREC_BY_NAME[prec_name]
    n, hi, cout = c["n"], c["hi"], c["cout"]
    a = L.IgemmArgs()
    a.x0, a.c0 = c["xd"].data_ptr(), c["cin"]
    a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride, a.resample = L.MODE_CONV3, n, hi, hi, 2 * hi, 2 * hi, 1, L.RS_UP2
    a.pro, a.pro_silu, a.pa, a.pb = L.PRO_AFFINE_NC, 1, c["pad"].data_ptr(), c["pbd"].data_ptr()
    a.cout, a.y_ld, a.prec, a.tune = cout, cout, p, L.TUNE_NO_SMALL
    sub = lib.sgd_igemm_subpixel_ok(C.byref(a)) == 1
    buf, cp, op, sinv = _pack(c["wd"], 3, p, sub=sub)
    if sub:
        a.resample = L.RS_UP2_SUBPIXEL
    y = torch.full((n, 2 * hi, 2 * hi, cout), float("nan"), device="cuda")
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias, a.y = buf.data_ptr(), cp, op, sinv.data_ptr(), c["bd"].data_ptr(), y.data_ptr()
    st = None
    if stats:
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts == 8
        st = torch.full((n, parts, 2, cout), float("nan"), device="cuda")
        a.stats = st.data_ptr()
    L.check(lib.sgd_igemm(C.byref(a), _st()), "igemm up")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2), (st.cpu() if st is not None else None), sub


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("stats", [False, True])
def test_subpixel_launch(stats, prec, tol):
    """n=2, 16x16 -> 32x32, 64 -> 128 as four 2x2 convs at the input resolution (parity-strided output rows, [parity][tile]
    statistics slots).  f32 has no sub-pixel instance (sgd_igemm_subpixel_ok refuses): there the direct SGD_RS_UP2 launch runs,
    as in the engine."""
    y, st, sub = run_up(prec, stats)
    assert sub == (prec != "f32")
    label = f"{'sub-pixel' if sub else 'direct up'} stats={stats} {prec}"
    check_output(y, up_case()["ref"], tol, label)
    if stats:
        check_stats(st, up_case()["ref"], tol, label)


_AUX = {}


def aux_case():
    if not _AUX:
        n, hw, cin, cout, ac = 2, 16, 64, 128, 32
        g = torch.Generator().manual_seed(59)
        h = torch.randn(n, cin, hw, hw, generator=g)
        xs = torch.randn(n, ac, hw, hw, generator=g)
        pa, pb = 1 + 0.3 * torch.randn(n, cin, generator=g), 0.3 * torch.randn(n, cin, generator=g)
        w3 = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
        w1 = torch.randn(cout, ac, 1, 1, generator=g) / math.sqrt(ac)
        b = torch.randn(cout, generator=g)
        act = F.silu(h.to(D) * pa.to(D)[:, :, None, None] + pb.to(D)[:, :, None, None])
        ref = F.conv2d(act, w3.to(D), b.to(D), padding=1) + F.conv2d(xs.to(D), w1.to(D))
        _AUX.update(n=n, hw=hw, cin=cin, cout=cout, ac=ac, ref=ref, hd=_nhwc(h).cuda(), xd=_nhwc(xs).cuda(), pad=pa.cuda(),
                    pbd=pb.cuda(), w3d=w3.cuda(), w1d=w1.reshape(cout, ac).contiguous().cuda(), bd=b.cuda())
    return _AUX


def run_aux(prec_name, stats):
    """-> (y NCHW cpu, statistics or None), or None where the mode has no fused-aux instance (query and launch refuse)"""
    L, lib = _lib()
    c = aux_case()
    p = L.PREC_BY_NAME[prec_name]
    n, hw, cout = c["n"], c["hw"], c["cout"]
    y = torch.full((n, hw, hw, cout), float("nan"), device="cuda")
    a = L.IgemmArgs()
    a.x0, a.c0 = c["hd"].data_ptr(), c["cin"]
    a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride = L.MODE_CONV3, n, hw, hw, hw, hw, 1
    a.pro, a.pro_silu, a.pa, a.pb = L.PRO_AFFINE_NC, 1, c["pad"].data_ptr(), c["pbd"].data_ptr()
    a.y, a.cout, a.y_ld, a.prec, a.tune = y.data_ptr(), cout, cout, p, L.TUNE_NO_SMALL
    xa = L.IgemmAux(x0=c["xd"].data_ptr(), x1=0, c0=c["ac"], c1=0)
    if lib.sgd_igemm_fused_aux_ok(C.byref(a), C.byref(xa)) != 1:
        assert lib.sgd_igemm_fused_aux(C.byref(a), C.byref(xa), _st()) == 1       # SGD_ERR_ARG, before any launch
        torch.cuda.synchronize()
        return None
    # both weight tensors back to back under ONE scale (as test_hip_fused_skip packs them)
    sizes = [int(lib.sgd_packed_weight_bytes(cout, c["cin"], 3, p)), int(lib.sgd_packed_weight_bytes(cout, c["ac"], 1, p))]
    buf = torch.empty(sum(sizes) // 4, device="cuda")
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    sinv = torch.ones(1, device="cuda")
    for w in (c["w3d"], c["w1d"]):
        L.check(lib.sgd_weight_amax(_p(w), w.numel(), _p(amax), _st()), "amax")
    cp, op, cp1, op1 = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    L.check(lib.sgd_pack_weight_scaled(_p(c["w3d"]), _p(buf), cout, c["cin"], 3, p, 0, _p(amax), _p(sinv), C.byref(cp), C.byref(op),
                                       _st()), "pack 3x3")
    L.check(lib.sgd_pack_weight_scaled(_p(c["w1d"]), C.c_void_p(buf.data_ptr() + sizes[0]), cout, c["ac"], 1, p, 0, _p(amax), _p(sinv),
                                       C.byref(cp1), C.byref(op1), _st()), "pack 1x1")
    a.w, a.cin_p, a.cout_p, a.w_scale_inv, a.bias = buf.data_ptr(), cp.value, op.value, sinv.data_ptr(), c["bd"].data_ptr()
    st = None
    if stats:
        parts = lib.sgd_igemm_stats_parts(C.byref(a))
        assert parts == 2
        st = torch.full((n, parts, 2, cout), float("nan"), device="cuda")
        a.stats = st.data_ptr()
    L.check(lib.sgd_igemm_fused_aux(C.byref(a), C.byref(xa), _st()), "fused aux")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2), (st.cpu() if st is not None else None)


@pytest.mark.parametrize("prec,tol", PRECS)
@pytest.mark.parametrize("stats", [False, True])
def test_fused_aux_launch(stats, prec, tol):
    """n=2, 16x16, 64 -> 128 with a 32-channel second input as extra K steps (sgd_igemm_fused_aux).  f32 has no such instance: the
    query and the launch refuse, before any launch."""
    got = run_aux(prec, stats)
    assert (got is None) == (prec == "f32")
    if got is None:
        return
    y, st = got
    label = f"fused aux stats={stats} {prec}"
    check_output(y, aux_case()["ref"], tol, label)
    if stats:
        check_stats(st, aux_case()["ref"], tol, label)
