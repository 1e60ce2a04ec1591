#!/usr/bin/env python3
"""Worst max|a - b| / max|b| against float64 of each attention core over its geometry sweep
(tests/test_hip_attention_geometry.py): one line per core, direction and head width -- what a rewrite of a core is compared
with, beyond the sweep's pass / fail.  With --cases also one line per launch.
    python tools/attention_geometry_errors.py  > profiles/attention_geometry_errors.txt   (MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import test_hip_attention_geometry as T  # noqa: E402

print("# worst max|a - b| / max|b| vs float64 over the 24 seeded launches of a sweep (tests/attention_refs.py: SWEEPS);")
print("# forward: out; backward: the worst of dq, dk, dv, each against its own maximum")
cases = []
for direction, run, table in (("forward", T.run_forward_sweep, T.FWD), ("backward", T.run_backward_sweep, T.BWD)):
    for kind in ("exact", "split", "masked"):
        core, tol = table[kind][0], table[kind][-1]
        worst, failures = run(kind, cases)
        for d, err in sorted(worst.items()):
            print(f"{core:26s} {direction:8s} d {d:3d}  worst {err:.2e}  (tolerance {tol:.0e})")
        for ci, cs, bad in failures:
            print(f"#   outside the sweep's checks: case {ci} {bad} {cs}")
if "--cases" in sys.argv:
    print("\n".join(cases))
