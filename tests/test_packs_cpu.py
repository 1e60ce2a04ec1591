"""sgdm_amd.packs without a GPU: the staleness rule on CPU tensors, and what a pack knows before its first refresh -- the padded
dims, the buffer size and whether PackBatch may re-pack it from a job table -- checked against the library's host-only entries."""
import ctypes as C

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from sgdm_amd import _lib as L
from sgdm_amd.packs import Derived, Packed, Stale, _Pad

# (cout, cin, ksize): both pick_bn branches (cout % 128 == 0 or not), a cin below one 32-channel chunk
SHAPES = [(40, 48, 1), (36, 20, 3), (128, 3, 3)]
SUBPIXEL = (64, 32, 3)


def _w(cout, cin, k):
    return torch.randn(cout, cin, k, k) if k == 3 else torch.randn(cout, cin)


# ---------------------------------------------------------------------------------------------- staleness
def test_stale_first_ask_mark_inplace_and_version_bump():
    p = torch.zeros(4, 3)
    st = Stale([p])
    assert st.changed()                                  # never marked
    st.mark()
    assert not st.changed() and not st.changed()
    p.add_(1.0)                                          # in-place op
    assert st.changed()
    st.mark()
    assert not st.changed()
    torch._C._increment_version([p])                     # what the fused optimizer does after writing through raw pointers
    assert st.changed()
    st.mark()
    assert not st.changed()


def test_stale_replaced_source_and_any_of_several():
    a, b, c = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    srcs = [a, b]
    st = Stale(srcs)
    st.mark()
    assert not st.changed()
    srcs[1] = c                                          # same version, same contents, another address
    assert c._version == b._version and c.data_ptr() != b.data_ptr()
    assert st.changed()
    st.mark()
    for t in (a, c):                                     # any one of them
        t.mul_(2.0)
        assert st.changed()
        st.mark()
        assert not st.changed()
    holder = dict(t=a)                                   # sources looked up at every ask
    st = Stale(lambda: (holder["t"],))
    st.mark()
    holder["t"] = b
    assert st.changed()


def test_stale_addresses_only_ignores_versions():
    a = torch.zeros(8)
    srcs = [a]
    st = Stale(srcs, versions=False)
    st.mark()
    a.add_(1.0)
    assert not st.changed()
    srcs[0] = torch.zeros(8)
    assert st.changed()


def test_derived_runs_its_update_only_when_a_source_changed():
    p, runs = torch.zeros(3), []

    def update(stream):
        runs.append(stream)
    d = Derived([p], update)
    assert d.__name__ == "update"
    assert d(7) == 0 and d(8) == 0 and runs == [7]
    p.add_(1.0)
    d.refresh(9)
    assert runs == [7, 9]


# ---------------------------------------------------------------------------------------------- construction
def _blocks(cout, cin, k, prec, kind):
    cp, op = C.c_int32(), C.c_int32()
    assert L.load().sgd_pack_job_blocks(cout, cin, k, prec, kind, None, None, C.byref(cp), C.byref(op)) == 0
    return cp.value, op.value


@pytest.mark.parametrize("prec", [L.PREC_F32, L.PREC_F16X3])
@pytest.mark.parametrize("cout,cin,k", SHAPES)
def test_forward_and_adjoint_dims_and_bytes(cout, cin, k, prec):
    lib, w = L.load(), _w(cout, cin, k)
    fwd = Packed([w], k, prec)
    assert (fwd.cin_p, fwd.cout_p) == _blocks(cout, cin, k, prec, L.PACK_FORWARD)
    assert fwd.buf.numel() * 4 == lib.sgd_packed_weight_bytes(cout, cin, k, prec)
    adj = Packed([w], k, prec, L.PACK_DGRAD, donor=fwd)
    assert (adj.cin_p, adj.cout_p) == _blocks(cout, cin, k, prec, L.PACK_DGRAD)
    assert adj.buf.numel() * 4 == lib.sgd_packed_weight_bytes(cin, cout, k, prec)      # the adjoint's outputs = cin
    assert adj.cin_p >= cout and adj.cout_p >= cin and fwd.cin_p >= cin and fwd.cout_p >= cout
    for pk in (fwd, adj):
        assert (pk.cout, pk.cin, pk.ksize, pk.subpixel, pk.idle, pk.pad) == (cout, cin, k, False, False, None)
        assert pk.scaled == (prec != L.PREC_F32) and (pk.scale_ptr != 0) == pk.scaled and pk.srcs[0] is w
        assert pk.stale.changed()                        # constructed, not packed


def test_subpixel_dims_and_bytes():
    cout, cin, k = SUBPIXEL
    pk = Packed([_w(cout, cin, k)], k, L.PREC_F16X3, L.PACK_SUBPIXEL)
    assert pk.subpixel and (pk.cin_p, pk.cout_p) == _blocks(cout, cin, k, L.PREC_F16X3, L.PACK_SUBPIXEL)
    assert pk.buf.numel() * 4 == L.load().sgd_packed_weight_subpixel_bytes(cout, cin, L.PREC_F16X3)


# ---------------------------------------------------------------------------------------------- batchability
@pytest.mark.parametrize("kind,cout,cin,k", [(L.PACK_FORWARD,) + SHAPES[0], (L.PACK_FORWARD,) + SHAPES[1], (L.PACK_DGRAD,) + SHAPES[0],
                                             (L.PACK_DGRAD,) + SHAPES[2], (L.PACK_SUBPIXEL,) + SUBPIXEL])
def test_whole_parameter_is_batchable_as_its_kind(kind, cout, cin, k):
    w = torch.nn.Parameter(_w(cout, cin, k))
    pk = Packed([w], k, L.PREC_F16X3, kind)
    job = pk.batch_job()
    assert job is not None
    assert (job.src, job.dst, job.cout, job.cin, job.ksize, job.transpose) == (w.data_ptr(), pk.buf.data_ptr(), cout, cin, k, kind)
    assert (job.amax_bits, job.scale_inv, job.own_amax) == (pk.amax.data_ptr(), pk.scale_inv.data_ptr(), 1)
    f32 = Packed([w], k, L.PREC_F32, L.PACK_DGRAD if kind == L.PACK_DGRAD else L.PACK_FORWARD).batch_job()
    assert (f32.amax_bits, f32.scale_inv, f32.own_amax) == (None, None, 0)


def test_what_is_not_batchable():
    a, b = torch.nn.Parameter(_w(40, 48, 1)), torch.nn.Parameter(_w(24, 48, 1))
    assert Packed([a, b], 1, L.PREC_F16X3).batch_job() is None                          # concat of two
    heads = _Pad(rows=[h * 16 + i for h in range(5) for i in range(8)], n_rows=80)
    assert Packed([a], 1, L.PREC_F16X3, pad=heads).batch_job() is None                  # zero-padded
    assert Packed([a], 1, L.PREC_F16X3, L.PACK_DGRAD, pad=heads).batch_job() is None
    cols = Packed([a, b], 1, L.PREC_F16X3, L.PACK_DGRAD, src_fn=lambda: torch.cat([a, b], 0)[:, 0:16], dims=(64, 16))
    assert cols.batch_job() is None                                                     # the FiLM adjoint's column slices
    one = Packed([a], 1, L.PREC_F16X3, L.PACK_DGRAD, src_fn=lambda: a[:, 0:16], dims=(40, 16))
    assert one.batch_job() is None                                                      # a column slice of one parameter
    assert Packed([a.detach().double()], 1, L.PREC_F16X3).batch_job() is None           # not fp32
    assert Packed([_w(48, 40, 1).t()], 1, L.PREC_F16X3).batch_job() is None             # not contiguous


def test_row_slice_view_is_batchable():
    """the head conv of a head= engine: rows [0, head) of out.2.weight, a contiguous view that shares the parameter's version"""
    w = torch.nn.Parameter(_w(6, 32, 3))
    v = w.detach()[:3]
    pk = Packed([v], 3, L.PREC_F16X3)
    job = pk.batch_job()
    assert job is not None and (job.src, job.cout, job.cin, job.transpose) == (w.data_ptr(), 3, 32, L.PACK_FORWARD)
    pk.mark()
    with torch.no_grad():
        w.mul_(2.0)
    assert pk.due()                                      # the view follows the parameter's version counter
    pk.idle = True
    assert not pk.due()
