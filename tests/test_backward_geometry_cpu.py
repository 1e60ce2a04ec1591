"""train.gemm_geometry: what the backward program's two adjoints (Backward.dx / dw) derive from a forward GEMM's descriptor.
The expected tuples are the arguments the backward's call sites spelled out by hand before the adjoints were derived:
(cout, cin, taps, rows, dgrad geometry (n, h, w) or None, zero_up).  No device, no library."""
import pytest

import conftest  # noqa: F401  (puts the package on sys.path)
from sgdm_amd import _lib as L
from sgdm_amd.train import gemm_geometry


def flat(m, c0, cout, c1=0):
    a = L.IgemmArgs()
    a.mode, a.m, a.stride, a.c0, a.c1, a.cout = L.MODE_FLAT, m, 1, c0, c1, cout
    return a


def conv(n, hi, wi, ho, wo, stride, resample, c0, cout, c1=0):
    a = L.IgemmArgs()
    a.mode, a.n, a.hi, a.wi, a.ho, a.wo, a.stride, a.resample = L.MODE_CONV3, n, hi, wi, ho, wo, stride, resample
    a.c0, a.c1, a.cout = c0, c1, cout
    return a


CASES = [
    # AttentionBlock.qkv at 2 x 4 x 4: wgrad(.., 96, 32, 1, n * T, ..), dgrad(.., m=n * T)
    ("flat", flat(2 * 16, 32, 96), (96, 32, 1, 32, None, False)),
    # a ResBlock's skip_connection over the virtual concat [h, skip]: cin = c0 + c1
    ("flat_two_sources", flat(2 * 16, 32, 64, c1=16), (64, 48, 1, 32, None, False)),
    # out_layers.3: wgrad(.., 9, n * ho * wo, ..), dgrad(.., conv=(n, ho, wo))
    ("conv3_stride1", conv(2, 8, 8, 8, 8, 1, L.RS_NONE, 32, 32), (32, 32, 9, 2 * 8 * 8, (2, 8, 8), False)),
    # Downsample.op 8 x 8 -> 4 x 4: dgrad(.., conv=(n, hh // 2, ww // 2), zero_up=True), rows n * (hh // 2) * (ww // 2)
    ("conv3_stride2", conv(2, 8, 8, 4, 4, 2, L.RS_NONE, 32, 32), (32, 32, 9, 2 * 4 * 4, (2, 4, 4), True)),
    # Upsample.conv 4 x 4 -> 8 x 8 (the DIRECT RS_UP2 descriptor): dgrad(.., conv=(n, 2 * hh, 2 * ww)), rows n * 4 * hh * ww
    ("conv3_up2", conv(2, 4, 4, 8, 8, 1, L.RS_UP2, 32, 32), (32, 32, 9, 2 * 8 * 8, (2, 8, 8), False)),
    # in_layers.2 of a down ResBlock 8 x 8 -> 4 x 4, two sources: everything at the output resolution, no zero_up
    ("conv3_avgpool2", conv(2, 8, 8, 4, 4, 1, L.RS_AVGPOOL2, 32, 64, c1=16), (64, 48, 9, 2 * 4 * 4, (2, 4, 4), False)),
]


@pytest.mark.parametrize("name,a,want", CASES, ids=[c[0] for c in CASES])
def test_gemm_geometry(name, a, want):
    g = gemm_geometry(a)
    assert tuple(g) == want
    assert (g.cout, g.cin, g.taps, g.rows, g.conv, g.zero_up) == want
