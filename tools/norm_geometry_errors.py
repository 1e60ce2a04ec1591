#!/usr/bin/env python3
"""Worst max|a - b| / max|b| against float64 of the GroupNorm / LayerNorm kernels over their geometry sweeps
(tests/test_hip_norm_geometry.py), one line per family and quantity next to its tolerance, and the mean-offset table of the
GroupNorm forward chain: our error of a x + b, the error of torch's fp32 CPU group_norm on the same input, the a-priori bound of
the one-pass variance and the margin the test applies.  With --cases also one line per launch or chain.
    python tools/norm_geometry_errors.py --cases > profiles/norm_geometry_errors.txt   (MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import test_hip_norm_geometry as T  # noqa: E402

print("# worst max|a - b| / max|b| vs float64 over the seeded cases of a sweep (tests/norm_refs.py: SWEEPS), MI355X")
cases = []
for family, run in (("A chan_stats", lambda: T.run_chan_stats_sweep(cases)), ("B partial statistics", lambda: T.run_parts_sweep(cases)),
                    ("C forward chain", lambda: T.run_gn_sweep("forward", cases)),
                    ("D backward chain", lambda: T.run_gn_sweep("backward", cases)),
                    ("E layernorm", lambda: T.run_layernorm_sweep("layernorm", cases)),
                    ("F degenerate groups", lambda: T.run_gn_sweep("degenerate", cases)),
                    ("F constant rows", lambda: T.run_layernorm_sweep("ln_degenerate", cases))):
    worst, failures = run()
    for nm, (err, tol) in worst.items():
        print(f"{family:22s} {nm:22s} worst {err:.2e}  (tolerance {tol:.0e})")
    for ci, cs, bad in failures:
        print(f"#   outside the sweep's checks: case {ci} {bad} {cs}")
print("# G mean offset: GroupNorm forward on x = r + randn, 32 channels in 8 groups; a x + b against float64.  a-priori bound:")
print("# relative error of rstd from one rounding to float of each sum, 2^-25 (1 + 3 r^2), at the data's own largest group r.")
print(f"# r <= 4: the standing {T.TOL['affine']:.0e} is asserted.  r >= 16: error <= {T.OFFSET_MARGIN:g} x bound is asserted.")
table = []
rows, failures = T.run_offset_sweep(table)
print("\n".join(table))
big = [err / bound for cs, err, _, bound, _ in rows if cs["r"] > 4]
print(f"# largest error / bound over r >= 16: {max(big):.2f}; margin in use: {T.OFFSET_MARGIN:g}")
worst_by_r = {}
for cs, err, _, _, _ in rows:
    worst_by_r[cs["r"]] = max(worst_by_r.get(cs["r"], 0.0), err)
inside = [r for r in sorted(worst_by_r) if all(worst_by_r[q] < 1e-4 for q in worst_by_r if q <= r)]
print(f"# a x + b stays inside the 1e-4 parity contract up to r = {max(inside)} of the measured r " + str(sorted(worst_by_r)))
for ci, cs, bad in failures:
    print(f"#   outside the sweep's checks: case {ci} {bad} {cs}")
if "--cases" in sys.argv:
    print("\n".join(cases))
