"""Global-norm gradient clipping (FusedAdamWEma(max_grad_norm=...), sgdm_amd.optim.clip_grad_norm_) where it needs no GPU: the
header declares the device record and the three entries, the binding mirrors them argument for argument, the ABI number stays,
and the optimizer's option validates its value before anything touches a device and stays out of the state dict."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import PKG, ROOT

ENTRIES = (("sgd_grad_norm", 8), ("sgd_grad_scale", 6), ("sgd_adamw_ema_clip_step", 16))


def _header():
    return open(os.path.join(ROOT, "include", "sgdm_hip.h")).read()


def _decl(txt, name):
    proto = re.search(r"^int %s\(([^;]*)\);" % name, txt, flags=re.M).group(1)
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]


def test_header_declares_the_record_and_the_three_entries():
    txt = _header()
    rec = re.search(r"typedef struct \{([^}]*)\} sgd_clip_record;", txt)
    assert rec, "sgd_clip_record is not declared"
    fields = re.findall(r"^\s*(float|int32_t)\s+(\w+)(\[\d+\])?;", rec.group(1), flags=re.M)
    assert [(t, n, d) for t, n, d in fields] == [("float", "norm", ""), ("float", "coef", ""), ("int32_t", "skip", ""),
                                                 ("int32_t", "clipped_steps", ""), ("int32_t", "nonfinite_steps", ""),
                                                 ("int32_t", "pad", "[3]")]
    for name, nargs in ENTRIES:
        decl = _decl(txt, name)
        assert len(decl) == nargs, (name, decl)
        assert decl[0].startswith("const sgd_opt_tensor*") and decl[1].startswith("const int32_t*"), name
        assert decl[-1] == "void* stream", name
        assert any("sgd_clip_record*" in d for d in decl), name
    # the clipped step is the plain step's argument list with the record put in front of the stream
    plain, clipped = _decl(txt, "sgd_adamw_ema_step"), _decl(txt, "sgd_adamw_ema_clip_step")
    assert [d.split()[-1] for d in clipped] == [d.split()[-1] for d in plain[:-1]] + ["rec", "stream"]
    assert "const sgd_clip_record* rec" in clipped and "const sgd_clip_record* rec" in _decl(txt, "sgd_grad_scale")
    assert "sgd_clip_record* rec" in _decl(txt, "sgd_grad_norm") and "double* partials" in _decl(txt, "sgd_grad_norm")


def test_binding_matches_the_header_and_the_abi_stays():
    from sgdm_amd import _lib as L
    txt = _header()
    assert int(re.search(r"#define SGD_ABI_VERSION (\d+)", txt).group(1)) == L.ABI_VERSION == 25
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    for name, nargs in ENTRIES:
        res, args = L.SIGNATURES[name]
        decl = _decl(txt, name)
        assert res is C.c_int32 and len(args) == len(decl) == nargs, name
        for a, d in zip(args, decl):
            if "*" in d:
                assert a in (C.c_void_p, L.dvp), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
        names = [d.split()[-1] for d in decl]
        for dev_only in ("partials", "rec"):                                # what the kernels dereference: never host memory
            if dev_only in names:
                assert args[names.index(dev_only)] is L.dvp, (name, dev_only)
    assert L.SIGNATURES["sgd_adamw_ema_clip_step"][1][:14] == L.SIGNATURES["sgd_adamw_ema_step"][1][:14]
    import importlib.util
    spec = importlib.util.spec_from_file_location("sgdm_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "gradclip.hip" in b._sources() and b.FILE_FLAGS["gradclip.hip"] == ["-ffp-contract=off"]
    assert "misc.hip" not in b.FILE_FLAGS                                   # the optimizer keeps the global flags


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, float("nan"), True, False, "1.0"])
def test_max_grad_norm_refuses(bad):
    from sgdm_amd.optim import FusedAdamWEma
    with pytest.raises(ValueError):
        FusedAdamWEma(_params(), max_grad_norm=bad)
    opt = FusedAdamWEma(_params())
    with pytest.raises(ValueError):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm is None                                        # a refused value leaves the old one


def test_max_grad_norm_is_an_attribute_not_a_group_key():
    from sgdm_amd.optim import FusedAdamWEma
    assert FusedAdamWEma(_params()).max_grad_norm is None
    for v in (1.0, 1, 0.25, float("inf")):
        opt = FusedAdamWEma(_params(), max_grad_norm=v)
        assert opt.max_grad_norm == float(v) and isinstance(opt.max_grad_norm, float)
        sd = opt.state_dict()
        assert "max_grad_norm" not in sd["param_groups"][0] and "max_grad_norm" not in opt.defaults
        assert sorted(sd) == ["param_groups", "state"]
        assert sd["param_groups"] == FusedAdamWEma(_params()).state_dict()["param_groups"]     # what it was without the option
    opt.max_grad_norm = None                                                # cleared at any time
    assert opt.max_grad_norm is None
    opt.max_grad_norm = 2
    assert opt.max_grad_norm == 2.0 and math.isinf(FusedAdamWEma(_params(), max_grad_norm=float("inf")).max_grad_norm)
    # a state dict saved with the option loads into an optimizer without it and back
    plain = FusedAdamWEma(_params())
    plain.load_state_dict(opt.state_dict())
    assert plain.max_grad_norm is None


def test_clip_grad_norm_refuses_what_the_kernels_cannot_read():
    from sgdm_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError):                                       # a CPU gradient: there is no CPU fallback
        clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError):
        clip_grad_norm_([p], float("nan"))
    q = torch.nn.Parameter(torch.zeros(4))                                  # nothing to measure: norm 0, nothing launched
    assert float(clip_grad_norm_([q], 1.0)) == 0.0
