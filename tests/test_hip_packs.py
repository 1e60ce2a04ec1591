"""sgdm_amd.packs on the device: what Packed / FusedPacked.refresh leave in the buffer and in scale_inv is byte-equal to the
direct ABI calls on the same tensor, a refresh repacks exactly when a source changed, and an adjoint pack that borrows its
forward pack's max |w| makes no amax launch and writes the same bytes."""
import ctypes as C

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from sgdm_amd import _lib as L
from sgdm_amd.packs import FusedPacked, Packed, _Pad, _ptr

pytestmark = pytest.mark.gpu

PRECS = ["f32", "f16x3", "bf16x3", "f16"]
SPLIT = PRECS[1:]
SHAPES = [(40, 48, 1), (36, 20, 3), (128, 3, 3)]                 # as tests/test_packs_cpu.py
ENTRIES = ["sgd_weight_amax", "sgd_weight_amax_subpixel", "sgd_pack_weight", "sgd_pack_weight_dgrad", "sgd_pack_weight_scaled",
           "sgd_pack_weight_subpixel_scaled"]


def _w(cout, cin, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(cout, cin, k, k, generator=g) if k == 3 else torch.randn(cout, cin, generator=g)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _direct(w, cout, cin, k, prec, kind, off=0, buf=None, amax=None, fold=()):
    """the ABI calls themselves on the fp32 device tensor w -> (buffer, scale_inv or None).  fold: further tensors whose max |w|
    goes into the same amax; off / buf / amax: pack behind an earlier one, under its amax"""
    lib, st = L.load(), _stream()
    cp, op = C.c_int32(), C.c_int32()
    if buf is None:
        nbytes = (lib.sgd_packed_weight_subpixel_bytes(cout, cin, prec) if kind == L.PACK_SUBPIXEL else
                  lib.sgd_packed_weight_bytes(*((cin, cout) if kind == L.PACK_DGRAD else (cout, cin)), k, prec))
        buf = torch.empty(nbytes // 4, device="cuda")
    dst = C.c_void_p(buf.data_ptr() + off)
    if prec == L.PREC_F32:
        fn = lib.sgd_pack_weight_dgrad if kind == L.PACK_DGRAD else lib.sgd_pack_weight
        L.check(fn(_ptr(w), dst, cout, cin, k, prec, C.byref(cp), C.byref(op), st), "pack")
        return buf, None
    sinv = torch.ones(1, device="cuda")
    if amax is None:
        amax = torch.zeros(1, dtype=torch.int32, device="cuda")
        if kind == L.PACK_SUBPIXEL:
            L.check(lib.sgd_weight_amax_subpixel(_ptr(w), cout, cin, _ptr(amax), st), "amax")
        for t in (w,) + tuple(fold) if kind != L.PACK_SUBPIXEL else ():
            L.check(lib.sgd_weight_amax(_ptr(t), t.numel(), _ptr(amax), st), "amax")
    if kind == L.PACK_SUBPIXEL:
        L.check(lib.sgd_pack_weight_subpixel_scaled(_ptr(w), dst, cout, cin, prec, _ptr(amax), _ptr(sinv), C.byref(cp), C.byref(op),
                                                    st), "pack")
    else:
        L.check(lib.sgd_pack_weight_scaled(_ptr(w), dst, cout, cin, k, prec, kind, _ptr(amax), _ptr(sinv), C.byref(cp),
                                           C.byref(op), st), "pack")
    return buf, sinv


def _same(pk, ref):
    buf, sinv = ref
    assert torch.equal(pk.buf.view(torch.int32), buf.view(torch.int32))
    assert (sinv is None) == (not pk.scaled)
    if sinv is not None:
        assert torch.equal(pk.scale_inv, sinv) and float(sinv) > 0


@pytest.fixture
def calls(monkeypatch):
    """the library's single-tensor pack and amax entries wrapped by counters"""
    lib, n = L.load(), {}

    def wrap(name, fn):
        def counted(*a):
            n[name] = n.get(name, 0) + 1
            return fn(*a)
        return counted
    for name in ENTRIES:
        monkeypatch.setattr(lib, name, wrap(name, getattr(lib, name)))
    return n


@pytest.mark.parametrize("kind", [L.PACK_FORWARD, L.PACK_DGRAD])
@pytest.mark.parametrize("cout,cin,k", SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_refresh_equals_direct_pack(prec, cout, cin, k, kind):
    prec, w = L.PREC_BY_NAME[prec], _w(cout, cin, k)
    pk = Packed([w], k, prec, kind)
    pk.refresh(_stream())
    _same(pk, _direct(w, cout, cin, k, prec, kind))


@pytest.mark.parametrize("prec", SPLIT)
def test_subpixel_refresh_equals_direct_pack(prec):
    prec, w = L.PREC_BY_NAME[prec], _w(64, 32, 3)
    pk = Packed([w], 3, prec, L.PACK_SUBPIXEL)
    pk.refresh(_stream())
    _same(pk, _direct(w, 64, 32, 3, prec, L.PACK_SUBPIXEL))


@pytest.mark.parametrize("prec", SPLIT)
def test_fused_refresh_equals_direct_packs(prec):
    """one amax over both tensors, the 1x1 units behind the 3x3 ones at off1, the summed bias"""
    prec = L.PREC_BY_NAME[prec]
    w3, w1, b3, b1 = _w(32, 64, 3, 1), _w(32, 32, 1, 2), torch.randn(32).cuda(), torch.randn(32).cuda()
    pk = FusedPacked(w3, w1, b3, b1, prec)
    pk.refresh(_stream())
    assert pk.off1 == L.load().sgd_packed_weight_bytes(32, 64, 3, prec)
    assert pk.buf.numel() * 4 == pk.off1 + L.load().sgd_packed_weight_bytes(32, 32, 1, prec)
    amax = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in (w3, w1):
        L.check(L.load().sgd_weight_amax(_ptr(t), t.numel(), _ptr(amax), _stream()), "amax")
    buf = torch.empty_like(pk.buf)
    _, s3 = _direct(w3, 32, 64, 3, prec, L.PACK_FORWARD, buf=buf, amax=amax)
    _, s1 = _direct(w1, 32, 32, 1, prec, L.PACK_FORWARD, off=pk.off1, buf=buf, amax=amax)
    assert torch.equal(s3, s1)
    _same(pk, (buf, s3))
    assert torch.equal(pk.bias, b3 + b1)
    one = Packed([w3], 3, prec)                                    # its dims are the 3x3 operator's
    assert (pk.cin_p, pk.cout_p) == (one.cin_p, one.cout_p)


@pytest.mark.parametrize("kind", [L.PACK_FORWARD, L.PACK_DGRAD])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_padded_heads_equal_direct_pack_of_the_padded_matrix(prec, kind):
    """3 heads of width 8 padded to 16: as rows (qkv-like, [24, 20] -> [48, 20]) and as columns (proj_out-like, [20, 24] -> [20, 48])"""
    prec, hmap = L.PREC_BY_NAME[prec], [h * 16 + i for h in range(3) for i in range(8)]
    for w, pad, (cout, cin) in ((_w(24, 20, 1), _Pad(rows=hmap, n_rows=48), (48, 20)),
                                (_w(20, 24, 1), _Pad(cols=hmap, n_cols=48), (20, 48))):
        pk = Packed([w], 1, prec, kind, pad=pad)
        assert (pk.cout, pk.cin) == (cout, cin)
        pk.refresh(_stream())
        wp = torch.zeros(cout, cin, device="cuda")
        if pad.rows is not None:
            wp[hmap] = w
        else:
            wp[:, hmap] = w
        _same(pk, _direct(wp, cout, cin, 1, prec, kind))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_concatenated_sources_equal_direct_pack_of_the_concat(prec):
    prec, a, b = L.PREC_BY_NAME[prec], _w(40, 48, 1, 1), _w(24, 48, 1, 2)
    pk = Packed([a, b], 1, prec)
    pk.refresh(_stream())
    _same(pk, _direct(torch.cat([a, b], 0), 64, 48, 1, prec, L.PACK_FORWARD))
    adj = Packed([a, b], 1, prec, L.PACK_DGRAD, src_fn=lambda: torch.cat([a, b], 0)[:, 16:48], dims=(64, 32))
    adj.refresh(_stream())
    _same(adj, _direct(torch.cat([a, b], 0)[:, 16:48].contiguous(), 64, 32, 1, prec, L.PACK_DGRAD))


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_refresh_repacks_only_what_changed(prec, calls):
    prec, (cout, cin, k) = L.PREC_BY_NAME[prec], SHAPES[1]
    p = torch.nn.Parameter(_w(cout, cin, k))
    pk = Packed([p], k, prec)
    pk.refresh(_stream())
    first = dict(calls)
    assert first == ({"sgd_pack_weight": 1} if prec == L.PREC_F32 else {"sgd_weight_amax": 1, "sgd_pack_weight_scaled": 1})
    pk.refresh(_stream())
    assert calls == first                                          # nothing changed: no call
    with torch.no_grad():
        p.mul_(1.0009765625)
    pk.refresh(_stream())
    assert calls == {name: 2 * c for name, c in first.items()}
    now = dict(calls)
    _same(pk, _direct(p.detach(), cout, cin, k, prec, L.PACK_FORWARD))
    calls.clear()
    calls.update(now)
    kept = pk.buf.clone()
    pk.idle = True
    with torch.no_grad():
        p.mul_(1.0009765625)
    pk.refresh(_stream())
    assert calls == now and torch.equal(pk.buf, kept)              # idle: left stale
    pk.idle = False
    pk.refresh(_stream())
    assert calls == {name: 3 * c for name, c in first.items()}


@pytest.mark.parametrize("cout,cin,k", SHAPES)
def test_adjoint_borrows_a_fresh_donors_amax(cout, cin, k, calls):
    prec = L.PREC_F16X3
    p = torch.nn.Parameter(_w(cout, cin, k))
    fwd = Packed([p], k, prec)
    lone, adj = Packed([p], k, prec, L.PACK_DGRAD), Packed([p], k, prec, L.PACK_DGRAD, donor=fwd)
    fwd.refresh(_stream())
    lone.refresh(_stream())
    assert calls == {"sgd_weight_amax": 2, "sgd_pack_weight_scaled": 2}
    adj.refresh(_stream())                                         # donor refreshed at this version: its max |w| is read
    assert calls == {"sgd_weight_amax": 2, "sgd_pack_weight_scaled": 3}
    _same(adj, (lone.buf, lone.scale_inv))
    # donor stale (the parameter moved on, the forward pack did not): the adjoint reduces its own
    with torch.no_grad():
        p.mul_(1.0009765625)
    lone.refresh(_stream())
    adj.refresh(_stream())
    assert calls == {"sgd_weight_amax": 4, "sgd_pack_weight_scaled": 5}
    _same(adj, (lone.buf, lone.scale_inv))
    _same(adj, _direct(p.detach(), cout, cin, k, prec, L.PACK_DGRAD))


def test_donors_that_do_not_lend(calls):
    """a sub-pixel pack (its amax is max |V|), a padded one, one of another tensor; an adjoint of a slice"""
    prec, st = L.PREC_F16X3, _stream()
    p, q = torch.nn.Parameter(_w(64, 32, 3)), torch.nn.Parameter(_w(64, 32, 3, 5))
    w1 = torch.nn.Parameter(_w(24, 20, 1))
    pad = _Pad(rows=[h * 16 + i for h in range(3) for i in range(8)], n_rows=48)
    cases = [(p, 3, Packed([p], 3, prec, L.PACK_SUBPIXEL), None, {}),
             (w1, 1, Packed([w1], 1, prec, pad=pad), pad, {}),
             (p, 3, Packed([q], 3, prec), None, {}),
             (p, 3, Packed([p], 3, prec), None, dict(src_fn=lambda: p[:32], dims=(32, 32)))]
    for w, k, donor, apad, kw in cases:
        donor.refresh(st)
        calls.clear()
        adj = Packed([w], k, prec, L.PACK_DGRAD, pad=apad, donor=donor, **kw)
        adj.refresh(st)
        assert calls == {"sgd_weight_amax": 1, "sgd_pack_weight_scaled": 1}
        lone = Packed([w], k, prec, L.PACK_DGRAD, pad=apad, **kw)
        lone.refresh(st)
        _same(adj, (lone.buf, lone.scale_inv))
