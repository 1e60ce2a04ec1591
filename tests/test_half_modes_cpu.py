"""The single-product inference modes ('f16', 'bf16') at the boundaries that need no GPU: the enum values of the C header and the
Python binding agree, every mode the binding names has its igemm translation unit (and the LayerNorm fence its no-packed-f32 twin),
the packed-weight size rule, and the training guard."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import PKG, ROOT


def _header_enum():
    txt = open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()
    return {k.lower(): int(v) for k, v in re.findall(r"SGD_PREC_(\w+) = (\d+)", txt)}, txt


def test_enum_values_agree_between_header_and_binding():
    from sgdm_amd import _lib as L
    enum, txt = _header_enum()
    assert enum == L.PREC_BY_NAME
    assert enum["f16"] == 3 and enum["bf16"] == 4
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    assert set(L.INFERENCE_ONLY) == {"f16", "bf16"}


def test_every_mode_has_its_translation_units():
    import importlib.util
    from sgdm_amd import _lib as L
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    units = dict(b.VARIANTS["igemm.hip"])
    for name, value in L.PREC_BY_NAME.items():
        assert f"-DSGDM_IGEMM_PREC={value}" in units["_" + name], name
        if name != "f32":                     # LayerNorm-row launches of every 16-bit mode: the unit without packed-f32 code
            flags = units["_" + name + "_nopk"]
            assert f"-DSGDM_IGEMM_PREC={value}" in flags and "-DSGDM_IGEMM_NOPK" in flags and "-packed-fp32-ops" in flags
    assert "-fno-slp-vectorize" in b.FILE_FLAGS["igemm.hip"]
    host = open(os.path.join(PKG, "csrc", "igemm_host.hip")).read()
    for name in L.PREC_BY_NAME:
        assert f"sgd_igemm_dispatch_{name}(" in host


def test_packed_weight_bytes_follow_the_mode():
    """host-only entry points: half the bytes of the x3 sibling (no lo half); unknown modes are refused by the pack planner"""
    from sgdm_amd import _lib as L
    try:
        lib = L.load()
    except Exception as e:                    # the library is a build product: __graft_entry__.build() makes it
        pytest.fail(f"libsgdm_hip.so does not load: {e}")
    for cout, cin, ks in ((512, 512, 3), (96, 40, 1), (3, 128, 3)):
        x3 = lib.sgd_packed_weight_bytes(cout, cin, ks, L.PREC_F16X3)
        assert x3 == lib.sgd_packed_weight_bytes(cout, cin, ks, L.PREC_BF16X3) == lib.sgd_packed_weight_bytes(cout, cin, ks, L.PREC_F32)
        assert lib.sgd_packed_weight_bytes(cout, cin, ks, L.PREC_F16) * 2 == x3
        assert lib.sgd_packed_weight_bytes(cout, cin, ks, L.PREC_BF16) * 2 == x3
    assert lib.sgd_packed_weight_subpixel_bytes(512, 512, L.PREC_F16) == 16 * 512 * 512 * 2
    i = C.c_int32
    outs = [i(), i(), i(), i()]
    refs = [C.byref(o) for o in outs]
    assert lib.sgd_pack_job_blocks(256, 128, 3, L.PREC_F16, L.PACK_SUBPIXEL, *refs) == 0
    assert lib.sgd_pack_job_blocks(256, 128, 3, 5, L.PACK_FORWARD, *refs) == 1


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_training_guard_names_the_mode(mode):
    from sgdm_amd.train import refuse_inference_only

    class M(torch.nn.Module):
        hip_precision = mode

    with pytest.raises(ValueError, match=f"hip_precision='{mode}' is inference only"):
        refuse_inference_only(torch.nn.Sequential(torch.nn.Identity(), M()))
    M.hip_precision = "f16x3"
    refuse_inference_only(M())
