#!/usr/bin/env python3
"""Two builds of the library over every launch of tests/test_hip_epilogue_paths.py IN ONE PROCESS: outputs and GroupNorm
statistic slots compared bit for bit (a change to the tile epilogue that keeps its arithmetic must print `same` everywhere).

    python tools/ab_epilogue_paths.py lib/libsgdm_hip_parent.so lib/libsgdm_hip.so
(paths relative to sgdm_amd/, as tools/ab_conv.py takes them)"""
import ctypes as C, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from sgdm_amd import _lib as L
import test_hip_epilogue_paths as T

LIBDIR = os.path.dirname(L.LIB_PATH)


def load(path):
    lib = C.CDLL(path if os.path.isabs(path) else os.path.join(os.path.dirname(LIBDIR), path))
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    return lib


def launches():
    """(label, thunk -> tuple of tensors / None) of every launch the test file makes"""
    P = [p for p, _ in T.PRECS]
    NS = L.TUNE_NO_SMALL
    for res, tile, st, p in itertools.product(T.RES_MODES, (128, 32), (False, True), P):
        yield f"3x3 n=3 16x16 32->128 res={res} tile={tile} stats={st} {p}", \
            lambda res=res, tile=tile, st=st, p=p: T.run_conv(T.conv_case(3, 16, 32, 128, res), p, tune=NS if tile == 128 else 0, stats=st)
    for res, p in itertools.product(("none", "same"), P):
        yield f"3x3 n=3 8x8 64->128 res={res} {p}", lambda res=res, p=p: T.run_conv(T.conv_case(3, 8, 64, 128, res), p, tune=NS)
    for cout, res, p in itertools.product((36, 35), T.RES_MODES, P):
        yield f"3x3 n=5 4x4 32->{cout} res={res} {p}", lambda cout=cout, res=res, p=p: T.run_conv(T.conv_case(5, 4, 32, cout, res), p)
    for cap, res, st, p in itertools.product((8, 16), ("none", "same"), (False, True), P):
        yield f"3x3 n=4 16x16 256->128 grid_cap={cap} workspace res={res} stats={st} {p}", \
            lambda cap=cap, res=res, st=st, p=p: T.run_conv(T.conv_case(4, 16, 256, 128, res), p, tune=NS, stats=st, grid_cap=cap, work=True)
    for tile, p in itertools.product(sorted(T.TILES), P):
        tune = getattr(L, T.TILES[tile]) if T.TILES[tile] else 0
        for res in (False, True):
            yield f"flat m=200 64->256 tile={tile} res={res} {p}", lambda tune=tune, res=res, p=p: T.run_flat(T.flat_case(200, 64, 256, res), p, tune)
        yield f"flat m=200 64->256 tile={tile} row remap {p}", lambda tune=tune, p=p: T.run_flat(T.flat_case(200, 64, 256, True), p, tune, remap=(8, 11, 2))
        yield f"flat m=256 64->256 tile={tile} stats {p}", \
            lambda tune=tune, p=p: T.run_flat(T.flat_case(256, 64, 256, True), p, tune, rows_per_n=128, stats=True)
    for st, p in itertools.product((False, True), P):
        yield f"up n=2 16x16->32x32 64->128 stats={st} {p}", lambda st=st, p=p: T.run_up(p, st)[:2]
        yield f"fused aux n=2 16x16 64->128 aux 32 stats={st} {p}", lambda st=st, p=p: T.run_aux(p, st)


def bits_equal(u, v):
    if u is None or v is None:
        return u is None and v is None
    return u.shape == v.shape and bool(torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)))


libs = [load(p) for p in sys.argv[1:3]]
ndiff = n = 0
for label, thunk in launches():
    outs = []
    for lib in libs:
        T._lib = lambda lib=lib: (L, lib)
        outs.append(thunk())
    a, b = outs
    same = (a is None and b is None) or (a is not None and b is not None and all(bits_equal(u, v) for u, v in zip(a, b)))
    n += 1; ndiff += not same
    print(f"{label}: {'same' if same else 'DIFFERENT'}", flush=True)
print(f"# {n} launches, {ndiff} differ between {sys.argv[1]} and {sys.argv[2]}")
