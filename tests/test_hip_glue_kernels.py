"""The small C-ABI entry points that so far ran only inside whole-UNet and whole-step goldens, each on its own through ctypes (as
test_hip_kernels.test_boundary_kernels does for its neighbours): the branches the goldens' shapes do not reach, the claims
include/sgdm_hip.h makes about them ("bit-identical to the dense product", "exactly as the reference's data workers expand it",
"truncation"), and -- through the guarded buffers of tests/attention_refs.py -- no write outside the owned rows and columns.
"exact" = torch.equal with the stated fp32 CPU computation; TOL = max_rel against float64 at the fp32 tolerance of the project."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from attention_refs import Guarded
from conftest import max_rel
from test_hip_kernels import PRECS

pytestmark = pytest.mark.gpu

TOL = PRECS[0][1]
assert PRECS[0][0] == "f32" and TOL == 2e-6


def _lib():
    from sgdm_amd import _lib as L
    return L, L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _nan_padded(t, ld):
    """[rows, c] -> [rows, ld] with NaN in the padding columns (an input's padding must never be read)"""
    out = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def _done(*bufs):
    torch.cuda.synchronize()
    for buf in bufs:
        assert buf.written(), "an owned element was not written"
        assert buf.untouched(), "a write outside the owned rows and columns"


# ---------------------------------------------------------------------------------------------------------------------
# sgd_pack_input_compact
# ---------------------------------------------------------------------------------------------------------------------
H, W, N_SRC, N, CX = 6, 10, 3, 6, 3            # a non-square frame: a swap of px and py shows


def _pack_compact(layout_dev, fmt, cl, expanded):
    """the compact launch against the host expansion `expanded` [N_SRC, cl, H, W]: exact, and byte for byte what sgd_pack_input
    makes of the expanded layout"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(N_SRC, CX, H, W, generator=g)
    nl = torch.randn(1, 1, H, W, generator=g)
    mask = torch.tensor([False, True, False, True, False, True])           # both values in each half of the doubled batch
    xd, nld, md, ed = x.cuda(), nl.cuda(), mask.to(torch.uint8).cuda(), expanded.cuda()
    ct = CX + cl
    out, out2 = Guarded(N * H * W, ct), Guarded(N * H * W, ct)
    L.check(lib.sgd_pack_input_compact(_p(xd), _p(layout_dev), fmt, _p(md), _p(nld), N_SRC, N, CX, cl, H, W, out.ptr, _stream()),
            "pack_input_compact")
    L.check(lib.sgd_pack_input(_p(xd), _p(ed), _p(md), _p(nld), N_SRC, N, CX, cl, H, W, out2.ptr, _stream()), "pack_input")
    _done(out, out2)
    xx, ll = torch.cat([x, x]), torch.cat([expanded, expanded])
    ref = torch.cat([xx, torch.where(mask[:, None, None, None], nl, ll)], 1).permute(0, 2, 3, 1).reshape(N * H * W, ct)
    assert torch.equal(out.owned(), ref)
    assert torch.equal(out.owned().view(torch.int32), out2.owned().view(torch.int32))


def test_pack_input_compact_label_map():
    """fmt 1: uint8 label map -> one-hot over cl channels, 255 -> class 0 (stego_to_onehotmask)"""
    cl = 5
    g = torch.Generator().manual_seed(22)
    labels = torch.tensor([0, 1, 2, 3, 4, 255], dtype=torch.uint8)[torch.randint(0, 6, (N_SRC, H, W), generator=g)]
    labels[0, 0, 0], labels[1, 2, 7], labels[2, H - 1, W - 1] = 255, 255, 255
    assert all(int((labels == v).sum()) > 0 for v in (0, 1, 2, 3, 4, 255))
    lab = torch.where(labels == 255, torch.zeros_like(labels), labels).long()
    expanded = F.one_hot(lab, cl).permute(0, 3, 1, 2).float().contiguous()
    _pack_compact(labels.cuda(), 1, cl, expanded)


@pytest.mark.parametrize("boxes", [[(0, 0, W, H), (3, 2, 3, 5), (7, 4, W, H)], [(4, 3, 5, 4), (0, 0, W, H), (7, 4, W, H)]],
                         ids=["full_empty_edges", "single_pixel_full_edges"])
def test_pack_input_compact_boxes(boxes):
    """fmt 2: int32 boxes (x0, y0, x1, y1) -> mask[y0:y1, x0:x1] = 1 (get_lostbboxmask): the full frame, an empty box
    (x0 == x1), one touching the right and bottom edges, a single pixel"""
    expanded = torch.zeros(N_SRC, 1, H, W)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        expanded[i, 0, y0:y1, x0:x1] = 1.0
    assert float(expanded[0].sum()) in (H * W, 1.0) and 0 < float(expanded[2].sum()) < H * W
    _pack_compact(torch.tensor(boxes, dtype=torch.int32).cuda(), 2, 1, expanded)


# ---------------------------------------------------------------------------------------------------------------------
# sgd_labelmap_nhot
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,hw,k", [(1, 1, 1), (3, 300, 27), (2, 4099, 256)])
def test_labelmap_nhot(b, hw, k):
    """out[b, j] = 1 iff label j occurs in map b; labels >= k are ignored (255 is a label like any other at k = 256)"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(23 + k)
    if k == 1:
        maps = [torch.tensor([[0]]), torch.tensor([[5]])]               # the one label present; only a label without a column
    else:
        rows = []
        for _ in range(b):                                               # each map draws from its own half of the labels ...
            alphabet = torch.randperm(k, generator=g)[:k // 2]
            alphabet[:2] = torch.tensor([255, 254] if k == 256 else [k, k + 3])      # ... and, k < 256, two without a column
            rows.append(alphabet[torch.randint(0, len(alphabet), (hw,), generator=g)])
        maps = [torch.stack(rows)]
    for labels in maps:
        out = Guarded(b, k)
        ld = labels.to(torch.uint8).cuda()
        L.check(lib.sgd_labelmap_nhot(_p(ld), b, hw, k, out.ptr, _stream()), "labelmap_nhot")
        _done(out)
        ref = torch.zeros(b, 256)
        ref.scatter_(1, labels, 1.0)
        assert torch.equal(out.owned(), ref[:, :k])
        if k > 1:
            assert 0 < float(ref[:, :k].sum()) < b * k and float(ref[:, k:].sum()) == (0 if k == 256 else 2 * b)
        assert lib.sgd_labelmap_nhot(_p(ld), b, hw, 257, out.ptr, _stream()) != 0, "present[] has 256 slots"


# ---------------------------------------------------------------------------------------------------------------------
# sgd_linear_gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("n_src,n,nout,k", [(3, 6, 96, 7), (2, 4, 257, 5000)])
def test_linear_gather(n_src, n, nout, k, with_bias):
    """y[r] = mask[r] ? nullproj : w[:, ids[r % n_src]] + bias, exact -- and, the header's claim, bit-identical to the dense product:
    to sgd_linear_sparse_rows on the one-hot int64 rows and to sgd_linear_splitk on the one-hot fp32 rows"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(24)
    ldo = nout + 4
    ids = torch.randint(0, k, (n_src,), generator=g)
    ids[0], ids[-1] = k - 1, 0
    mask = torch.zeros(n, dtype=torch.bool)
    mask[1], mask[n - 2] = True, True
    w = torch.randn(nout, k, generator=g)
    bias = torch.randn(nout, generator=g) if with_bias else None
    nullproj = torch.randn(nout, generator=g)
    idd, md, wd, npd = ids.cuda(), mask.to(torch.uint8).cuda(), w.cuda(), nullproj.cuda()
    bd = bias.cuda() if with_bias else None
    out = Guarded(n, ldo, nout)
    L.check(lib.sgd_linear_gather(_p(idd), _p(md), _p(wd), _p(bd), _p(npd), n_src, n, nout, k, out.ptr, ldo, _stream()), "gather")
    _done(out)
    rows = ids[torch.arange(n) % n_src]
    ref = w[:, rows].t() + (bias if with_bias else torch.zeros(nout))
    ref = torch.where(mask[:, None], nullproj[None], ref)
    assert torch.equal(out.owned(), ref)
    # the dense routes
    onehot = F.one_hot(ids, k)
    ohd = onehot.cuda()
    sparse = Guarded(n, ldo, nout)
    L.check(lib.sgd_linear_sparse_rows(_p(ohd), _p(md), _p(wd), _p(bd), _p(npd), n_src, n, nout, k, sparse.ptr, ldo, _stream()),
            "sparse_rows")
    _done(sparse)
    assert torch.equal(sparse.owned().view(torch.int32), out.owned().view(torch.int32))
    xd = onehot[torch.arange(n) % n_src].float().cuda()
    keep = ~mask
    for ksplit in (1, 5):
        work = torch.full((ksplit, n, nout), float("nan"), device="cuda")
        dense = Guarded(n, ldo, nout)
        L.check(lib.sgd_linear_splitk(_p(xd), k, _p(wd), _p(bd), n, nout, k, _p(work), ksplit, dense.ptr, ldo, _stream()), "splitk")
        _done(dense)
        assert torch.equal(dense.owned()[keep].view(torch.int32), out.owned()[keep].view(torch.int32)), ksplit


def test_linear_gather_id_out_of_range():
    """an id outside [0, k) has no one-hot row: that row is NaN, nothing else changes, nothing is read out of bounds"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(25)
    n_src, n, nout, k, ldo = 3, 6, 96, 7, 100
    w, bias = torch.randn(nout, k, generator=g), torch.randn(nout, generator=g)
    wd, bd = w.cuda(), bias.cuda()
    for bad in (k, -1, 1 << 40):
        ids = torch.tensor([2, bad, 5])
        idd = ids.cuda()
        out = Guarded(n, ldo, nout)
        L.check(lib.sgd_linear_gather(_p(idd), None, _p(wd), _p(bd), None, n_src, n, nout, k, out.ptr, ldo, _stream()), "gather")
        _done(out)
        got = out.owned()
        assert torch.isnan(got[[1, 4]]).all()
        assert torch.equal(got[[0, 3]], (w[:, 2] + bias).expand(2, nout)) and torch.equal(got[[2, 5]], (w[:, 5] + bias).expand(2, nout))


# ---------------------------------------------------------------------------------------------------------------------
# sgd_linear_splitk_t
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,ksplit", [(1, 1, 1, 1), (33, 65, 31, 1), (80, 768, 1000, 7), (256, 64, 33, 5)])
def test_linear_splitk_t(m, n, k, ksplit):
    """y = x[m, :k] w[:k, window of n columns] against float64: ragged m / n / k, padded strides on x, w (read through a column
    window) and y, and -- (256, 64, 33, 5): 32-wide K slices of 33 rows -- K slices 2..4 empty"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(26)
    x_ld, w_ld, y_ld, off = k + 3, n + 8, n + 2, 4
    x = torch.randn(m, k, generator=g)
    w = torch.randn(k, n, generator=g) / k ** 0.5
    wfull = torch.full((k, w_ld), float("nan"))
    wfull[:, off:off + n] = w
    xd, wd = _nan_padded(x, x_ld).cuda(), wfull.cuda()
    work = torch.full((ksplit, m, n), float("nan"), device="cuda")
    y = Guarded(m, y_ld, n)
    wp = C.c_void_p(wd.data_ptr() + 4 * off)
    L.check(lib.sgd_linear_splitk_t(_p(xd), x_ld, wp, w_ld, m, n, k, _p(work), ksplit, y.ptr, y_ld, _stream()), "splitk_t")
    _done(y)
    assert torch.isfinite(work).all()
    assert max_rel(y.owned(), x.double() @ w.double()) < TOL
    assert lib.sgd_linear_splitk_t(_p(xd), x_ld, wp, w_ld, 257, n, k, _p(work), ksplit, y.ptr, y_ld, _stream()) != 0
    assert lib.sgd_linear_splitk_t(_p(xd), x_ld, wp, n - 1, m, n, k, _p(work), ksplit, y.ptr, y_ld, _stream()) != 0


# ---------------------------------------------------------------------------------------------------------------------
# sgd_token_pool
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [0, 1])
@pytest.mark.parametrize("n,tokens,c", [(5, 1, 52), (5, 16, 52), (3, 77, 260)])
def test_token_pool(n, tokens, c, cls):
    """cls = 1: token 0, exact.  cls = 0: the mean over the tokens as an fp32 running sum and one division, held element by
    element to that computation's analytic error, |err| <= tokens 2^-24 mean_t |x| + 2^-24 |ref| (every one of the tokens - 1
    additions rounds a partial sum of magnitude <= sum_t |x| by at most 2^-24 of it; the division adds 2^-24 |ref|).  A
    sequential fp32 sum of such inputs on the CPU stays below 0.12 of the bound: no measured tolerance is involved."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(27)
    cond = torch.randn(n, tokens, c, generator=g) * 3 + 0.5
    cd = cond.cuda()
    out = Guarded(n, c)
    L.check(lib.sgd_token_pool(_p(cd), n, tokens, c, cls, out.ptr, _stream()), "token_pool")
    _done(out)
    if cls:
        assert torch.equal(out.owned(), cond[:, 0])
        return
    ref = cond.double().mean(1)
    bound = tokens * 2.0 ** -24 * cond.double().abs().mean(1) + 2.0 ** -24 * ref.abs()
    err = (out.owned().double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# sgd_geglu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,inner", [(1, 4), (37, 20), (5, 1280)])
def test_geglu(rows, inner):
    """out = a * gelu_erf(gate) against float64, gates of 4 randn with the zeros, both tails and the cancelling region planted"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(28)
    x = torch.randn(rows, 2 * inner, generator=g)
    gate = 4 * torch.randn(rows, inner, generator=g)
    plant = torch.tensor([-5.0, 30.0, 0.0, -0.0, 10.0, -10.0])[:min(6, rows * inner)]
    gate.view(-1)[torch.randperm(rows * inner, generator=g)[:len(plant)]] = plant
    x[:, inner:] = gate
    xd = x.cuda()
    out = Guarded(rows, inner)
    L.check(lib.sgd_geglu(_p(xd), rows, inner, out.ptr, _stream()), "geglu")
    _done(out)
    a, gd = x[:, :inner].double(), gate.double()
    ref = a * (0.5 * gd * (1.0 + torch.erf(gd / math.sqrt(2.0))))
    assert max_rel(out.owned(), ref) < TOL
    assert lib.sgd_geglu(_p(xd), 1, 6, out.ptr, _stream()) != 0, "inner % 4 != 0"


# ---------------------------------------------------------------------------------------------------------------------
# sgd_to_uint8
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 257, 769])
def test_to_uint8(count):
    """exact against fp32 ((x + 1) * 127.5).clamp(0, 255).to(uint8) at every one of the 256 boundaries k / 127.5 - 1, the fp32
    numbers next to them on both sides, and values outside [-1, 1]: the image writer's rounding, bit for bit"""
    L, lib = _lib()
    edge = torch.arange(256, dtype=torch.float32) / 127.5 - 1.0
    near = torch.stack([torch.nextafter(edge, torch.tensor(-4.0)), edge, torch.nextafter(edge, torch.tensor(4.0))], 1).reshape(-1)
    if count == 769:
        x = torch.cat([near, torch.tensor([-1.5])])
    elif count == 257:
        x = torch.cat([near[1::3], torch.tensor([1.25])])                 # the boundaries themselves
    else:
        x = torch.tensor([3.0e9])
    assert x.numel() == count
    guard = 64
    buf = torch.full((count + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    xd = x.cuda()
    L.check(lib.sgd_to_uint8(_p(xd), count, C.c_void_p(buf.data_ptr() + guard), _stream()), "to_uint8")
    torch.cuda.synchronize()
    got = buf.cpu()
    assert bool((got[:guard] == 0xA5).all()) and bool((got[guard + count:] == 0xA5).all()), "a write outside the count bytes"
    ref = ((x + 1.0) * 127.5).clamp(0, 255).to(torch.uint8)
    assert torch.equal(got[guard:guard + count], ref), x[got[guard:guard + count] != ref]


# ---------------------------------------------------------------------------------------------------------------------
# sgd_add_rows_nc
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c", [(1, 1, 4), (3, 17, 36), (2, 64, 128)])
def test_add_rows_nc(n, hw, c):
    """x[n, hw, c] += e[n, c] in place, e with a padded row stride: one fp32 add, exact"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(29)
    e_ld = c + 8
    x, e = torch.randn(n, hw, c, generator=g), torch.randn(n, c, generator=g)
    ed = _nan_padded(e, e_ld).cuda()
    buf = Guarded(n * hw, c)
    buf.tensor().copy_(x.reshape(n * hw, c))
    L.check(lib.sgd_add_rows_nc(buf.ptr, _p(ed), e_ld, n, hw, c, _stream()), "add_rows_nc")
    _done(buf)
    assert torch.equal(buf.owned().view(n, hw, c), x + e[:, None])
    assert lib.sgd_add_rows_nc(buf.ptr, _p(ed), e_ld, n, hw, 6, _stream()) != 0, "c % 4 != 0"


# ---------------------------------------------------------------------------------------------------------------------
# sgd_cfg_combine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_mode", [0, 1, 2])
@pytest.mark.parametrize("b,c,hw", [(1, 3, 5), (3, 4, 64)])
def test_cfg_combine(b, c, hw, cfg_mode):
    """NHWC [2b | b, hw, c] -> guided NCHW [b, c, hw] by the header's two formulas, in float64; mode 0 is a transpose, exact"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(30)
    w = 2.5
    eps = torch.randn((2 * b if cfg_mode else b), hw, c, generator=g)
    ed = eps.cuda()
    out = Guarded(b * c, hw)
    L.check(lib.sgd_cfg_combine(_p(ed), cfg_mode, w, b, c, hw, out.ptr, _stream()), "cfg_combine")
    _done(out)
    got = out.owned().view(b, c, hw)
    e64 = eps.double().permute(0, 2, 1)
    if cfg_mode == 0:
        assert torch.equal(got, eps.permute(0, 2, 1))
        return
    ec, eu = e64[:b], e64[b:]
    ref = (1 - w) * eu + w * ec if cfg_mode == 1 else (1 + w) * ec - w * eu
    assert max_rel(got, ref) < TOL


# ---------------------------------------------------------------------------------------------------------------------
# sgd_fill_null_kv
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [16, 64])
@pytest.mark.parametrize("row", [0, 4])
def test_fill_null_kv(row, d):
    """kv[b, row] = [null_kv[0] | null_kv[1]] exactly, every other row of kv unchanged"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(31)
    batch, rows_per_b = 3, 5
    kv = torch.arange(batch * rows_per_b * 2 * d, dtype=torch.float32).reshape(batch * rows_per_b, 2 * d) + 0.5
    null_kv = torch.randn(2, d, generator=g)
    nd = null_kv.cuda()
    buf = Guarded(batch * rows_per_b, 2 * d)
    buf.tensor().copy_(kv)
    L.check(lib.sgd_fill_null_kv(_p(nd), batch, rows_per_b, row, d, buf.ptr, _stream()), "fill_null_kv")
    _done(buf)
    ref = kv.clone().view(batch, rows_per_b, 2 * d)
    ref[:, row] = null_kv.reshape(2 * d)
    assert torch.equal(buf.owned().view(batch, rows_per_b, 2 * d), ref)
    assert lib.sgd_fill_null_kv(_p(nd), batch, rows_per_b, rows_per_b, d, buf.ptr, _stream()) != 0, "row outside the batch element"


# ---------------------------------------------------------------------------------------------------------------------
# sgd_silu_bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 1025])
def test_silu_bwd(count):
    """gx = g SiLU'(x) = g s (1 + x (1 - s)), s = sigmoid(x), against float64; x = 6 randn with 0 and both saturated ends
    planted; exactly `count` elements are written"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(32)
    x, gy = 6 * torch.randn(count, generator=g), torch.randn(count, generator=g)
    plant = torch.tensor([0.0, 20.0, -20.0])[:min(3, count)]
    x[torch.randperm(count, generator=g)[:len(plant)]] = plant
    xd, gd = x.cuda(), gy.cuda()
    out = Guarded(1, count)
    L.check(lib.sgd_silu_bwd(_p(xd), _p(gd), count, out.ptr, _stream()), "silu_bwd")
    _done(out)
    s = torch.sigmoid(x.double())
    ref = gy.double() * s * (1 + x.double() * (1 - s))
    assert max_rel(out.owned().view(-1), ref) < TOL
