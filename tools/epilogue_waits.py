#!/usr/bin/env python3
"""Instruction-level check of the conv kernel's tile epilogue (no GPU needed): compile single instances of
csrc/igemm.hip (SGDM_DEV_ONE) to gfx950 assembly with the production flags and print, per epilogue variant, the
`s_waitcnt` instructions that carry a vmcnt field between the first and the last tile-output store, and the number of
flat loads.

    python tools/epilogue_waits.py [--src PATH/igemm.hip] [--only NAME ...] [--jobs N] [--keep DIR]

A store counts in vmcnt, so a `vmcnt(0)` between two output stores makes the second wait for the first one's
acknowledgement: a serial round trip per store.  A flat load can only be waited for with vmcnt(0) lgkmcnt(0).

How to read the output.  The epilogue variants (residual mode x split-tile finisher, 16-byte and scalar path) are
inlined into the kernel one after the other; a "group" (one line below) is a stretch of code with output stores in it
that no MFMA, barrier, unconditional branch or program end interrupts -- one variant, or one unrolled part of it.
Identical consecutive groups and identical consecutive stores are run-length encoded (`n x`).  Each store is written as

    [events ST]        the events since the store before it, IN PROGRAM ORDER, separated by `|`:
                       Ln = n global / buffer / flat loads in a row; otherwise the operands of an s_waitcnt with a vmcnt
                       field (a wait that repeats the one before it with no load between them is dropped)
                       ST4 = global_store_dwordx4 (16-byte path: tile outputs and GroupNorm statistic slots),
                       ST1 = global_store_dword (scalar path)

`[L16 | vmcnt(0) ST4]` is a batch whose 16 loads are in flight together and waited for once; `[L1 | vmcnt(0) | L1 | vmcnt(0) ..`
is a serial load round trip per load.  A `!` marks a store with a vmcnt wait BEFORE any load of its step: that wait can only
be for the acknowledgement of earlier stores.  The header counts, for the 16-byte and the scalar path apart, the stores, the
flagged ones (the first store of a group included) and the waits that follow loads (exposed load round trips, whole kernel).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-guided-diffusion-models_amd")
sys.path.insert(0, PKG)
import build as B  # noqa: E402

# (name, -DSGDM_IGEMM_PREC, TAPS (SGDM_DEV_ONE), BN, AUX[, VEC])
INSTANCES = [
    ("f16x3 3x3 BN=128", 1, 9, 128, False),
    ("f16x3 3x3 BN=128 AUX", 1, 9, 128, True),
    ("f16x3 3x3 BN=256", 1, 9, 256, False),
    ("f16x3 sub-pixel (TAPS=4) BN=128", 1, 4, 128, False),
    ("f16x3 1x1 BN=128", 1, 1, 128, False),
    ("f16x3 1x1 BN=256", 1, 1, 256, False),
    ("f16x3 1x1 BN=32", 1, 1, 32, False),
    ("bf16x3 3x3 BN=128", 2, 9, 128, False),
    ("f32 3x3 BN=128", 0, 9, 128, False),
    # not in the issue's list: the scalar-input twin of the first instance (the one without a register to spare)
    ("f16x3 3x3 BN=128 scalar inputs (VEC=false)", 1, 9, 128, False, False),
]

SPLIT = re.compile(r"^\s*(v_mfma|s_barrier|s_branch|s_endpgm|s_setpc)")
WAIT = re.compile(r"^\s*s_waitcnt\s+(.*?)\s*(;.*)?$")


def compile_asm(src, inst, out):
    name, prec, taps, bn, aux = inst[:5]
    vec = inst[5] if len(inst) > 5 else True
    cmd = [B.HIPCC, *[f for f in B.FLAGS if f != "-fPIC"], *B.FILE_FLAGS["igemm.hip"], f"-DSGDM_IGEMM_PREC={prec}",
           f"-DSGDM_DEV_ONE={taps}", f"-DSGDM_DEV_BN={bn}", "-DSGDM_DEV_DEFER=false", f"-DSGDM_DEV_AUX={'true' if aux else 'false'}",
           f"-DSGDM_DEV_VEC={'true' if vec else 'false'}", *os.environ.get("SGDM_EXTRA_FLAGS", "").split(),
           "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {name}:\n{r.stderr}")
    return out


def groups_of(asm):
    """[steps]: steps = [(events since the previous store, store kind)]; events, in program order, are ("L", n) -- n global /
    buffer / flat loads in a row -- and ("W", operands) -- an s_waitcnt with a vmcnt field.  A wait that repeats the one
    before it with no load between them is dropped (nothing new is pending)."""
    out, steps, ev = [], [], []
    flat = 0
    for line in asm.splitlines():
        if SPLIT.match(line):
            if steps:
                out.append(steps)
            steps, ev = [], []
            continue
        s = line.strip()
        if s.startswith("global_store_dwordx4") or s.startswith("global_store_dword "):
            steps.append((tuple(ev), "ST4" if "dwordx4" in s else "ST1"))
            ev = []
        elif s.startswith(("global_load", "buffer_load", "flat_load")):
            flat += s.startswith("flat_load")
            if ev and ev[-1][0] == "L":
                ev[-1] = ("L", ev[-1][1] + 1)
            else:
                ev.append(("L", 1))
        else:
            m = WAIT.match(line)
            if m and "vmcnt" in m.group(1) and not (ev and ev[-1] == ("W", m.group(1))):
                ev.append(("W", m.group(1)))
    if steps:
        out.append(steps)
    return out, flat


def rle(items, fmt):
    parts, i = [], 0
    while i < len(items):
        j = i
        while j < len(items) and items[j] == items[i]:
            j += 1
        parts.append((f"{j - i} x " if j - i > 1 else "") + fmt(items[i]))
        i = j
    return parts


def store_waits(ev):
    """waits of a step with no load issued before them since the store before: they can only be for earlier stores"""
    n = 0
    for kind, _ in ev:
        if kind == "L":
            break
        n += 1
    return n


def load_trips(ev):
    """waits of a step that follow loads: exposed load round trips"""
    return sum(1 for i, (kind, _) in enumerate(ev) if kind == "W" and i > 0 and ev[i - 1][0] == "L")


def render(steps):
    def one(st):
        ev, k = st
        toks = [f"L{v}" if kind == "L" else v for kind, v in ev]
        return "[" + " | ".join(toks) + (" " if toks else "") + ("!" if store_waits(ev) else "") + k + "]"
    return "  ".join(rle(steps, one))


def report(inst, asm):
    lines = [f"== {inst[0]}"]
    gs, flat = groups_of(asm)
    meta = {k: (re.search(r"\." + k + r":\s+(\S+)", asm) or [None, "?"])[1]
            for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    st4 = [ev for steps in gs for ev, k in steps if k == "ST4"]
    st1 = [ev for steps in gs for ev, k in steps if k == "ST1"]
    lines.append(f"   flat_load: {flat}   ST4: {len(st4)} stores, {sum(1 for e in st4 if store_waits(e))} flagged `!`, "
                 f"{sum(load_trips(e) for e in st4)} waits behind loads   ST1: {len(st1)} stores, {sum(1 for e in st1 if store_waits(e))} "
                 f"flagged, {sum(load_trips(e) for e in st1)} waits behind loads   (vgpr {meta['vgpr_count']} vspill "
                 f"{meta['vgpr_spill_count']} scratch {meta['private_segment_fixed_size']})")
    for g in rle([render(steps) for steps in gs], lambda r: r):
        lines.append("   " + g)
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(PKG, "csrc", "igemm.hip"))
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="directory that keeps the .s files")
    a = ap.parse_args()
    insts = [i for i in INSTANCES if not a.only or any(o in i[0] for o in a.only)]
    if "SGDM_DEV_VEC" not in open(a.src).read():      # a tree whose development switch compiles 16-byte-input instances only
        insts = [i for i in insts if len(i) < 6 or i[5]]
    tmp = a.keep or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    with ThreadPoolExecutor(max_workers=a.jobs) as ex:
        outs = list(ex.map(lambda ki: compile_asm(a.src, ki[1], os.path.join(tmp, f"inst{ki[0]}.s")), enumerate(insts)))
    for inst, path in zip(insts, outs):
        with open(path) as f:
            print(report(inst, f.read()), flush=True)
        if not a.keep:
            os.remove(path)


if __name__ == "__main__":
    main()
