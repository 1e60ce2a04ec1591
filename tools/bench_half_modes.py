#!/usr/bin/env python3
"""The captured sampling step of bench.py's workloads in several arithmetic modes, in ONE process, alternating.

bench.py cannot time the single-product modes (its dtype / peak tables know three names), so this tool imports it as
tools/bench_samplers.py does, builds the same workload (bench.build_model, same seeds, same batch) and times the same call --
W untimed warm-up steps, then K steps of LatentDiffusion's native sampler on the hipGraph-captured step, synchronised wall clock --
for every precision of --precs, `--rounds` times in an order that alternates them (a b c a b c ...), so clock drift and other
tenants of the box hit all modes alike.  Prints one line per measurement, then medians and spreads (max - min) per mode and
the ratio to the first mode.  K and W default to a plain bench.py run's.

    python tools/bench_half_modes.py --workload c2 [--precs f16x3,f16,bf16] [--rounds 3] [--steps 10] [--warmup 3] [--out FILE]
    python tools/bench_half_modes.py --workload c2 --free-run 8      # + 1000-step trajectories at batch 8: image distance to f32

--free-run B records (does not judge) what a whole free-running native trajectory does to the final image in each mode: rel-L2 of
the final image and the share of differing uint8 pixels against the f32 mode from the same x_T and noise; a seeded-random-weight
UNet gives no meaningful image distance, so f16x3 is listed as the scale to read the others by.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch  # noqa: E402

import bench  # noqa: E402


class Leg:
    """one precision of the workload: model, diffusion wrapper, static inputs -- bench.py main()'s set-up"""

    def __init__(self, wl, prec, B):
        from sgdm_amd.diffusion import LatentDiffusion
        self.prec, self.B, self.S = prec, B, wl["image"]
        self.model, _, data = bench.build_model(wl, "cuda", prec, B)
        self.diff = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
        self.diff.set_denoise_fn(self.model.forward, self.model.forward_with_cond_scale)
        cond = data.get("cond")
        if cond is not None:
            cond = cond.cuda() if wl["kind"] == "unet_fast" else cond.float().cuda()
        layout = data["layout"].cuda() if "layout" in data else None
        self.dkw = dict(cond=cond, layout=layout, cond_scale=2.0)
        self.skw = dict(sampling_method="native", num_timesteps=1000, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True,
                        dtp=1, temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True,
                        hip_graph=True)
        torch.manual_seed(23)
        self.x = torch.randn(B, 3, self.S, self.S, device="cuda")

    def run_steps(self, x, idx):
        img, _ = self.diff.sampler.sample((self.B, 3, self.S, self.S), sampling_kwargs=self.skw,
                                          denoise_sample_fn=self.diff.denoise_sample_fn, denoise_sample_fn_kwargs=self.dkw,
                                          x_T=x, step_indices=idx)
        return img

    def setup(self):
        with torch.no_grad():
            self.run_steps(self.x.clone(), [999])           # launch program, workspace, weight packs, graph capture: untimed
        torch.cuda.synchronize()

    def measure(self, steps, warmup):
        """ms per step: bench.py's timed window"""
        with torch.no_grad():
            x = self.run_steps(self.x, [(999 - i) % 1000 for i in range(warmup)]) if warmup else self.x
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = self.run_steps(x, [(999 - i) % 1000 for i in range(warmup, warmup + steps)])
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / steps
        assert torch.isfinite(x).all(), self.prec
        return ms


def free_run(wl, precs, B, lines):
    """whole 1000-step native trajectories from one x_T / one noise stream per mode; distances to the f32 mode's final image"""
    finals = {}
    for prec in ["f32"] + [p for p in precs if p != "f32"]:
        leg = Leg(wl, prec, B)
        with torch.no_grad():
            torch.manual_seed(99)
            img = leg.run_steps(leg.x.clone(), list(range(999, -1, -1)))
        torch.cuda.synchronize()
        assert torch.isfinite(img).all(), prec
        finals[prec] = img.float().cpu()
        del leg
        torch.cuda.empty_cache()
    u8 = lambda t: ((t.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)
    ref = finals["f32"]
    lines.append(f"# free-running native-1000 at batch {B} (UNet batch {2 * B}), same x_T and noise: final image against the f32 mode (recorded, not judged)")
    for prec, img in finals.items():
        if prec == "f32":
            continue
        rl2 = float((img - ref).double().norm() / ref.double().norm())
        share = float((u8(img) != u8(ref)).float().mean())
        lines.append(f"free_run {prec:7s} rel_l2 {rl2:.3e}  uint8 pixels differing {share:.2%}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--precs", default="f16x3,f16,bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--free-run", type=int, default=0, metavar="B")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sgdm_amd import _lib as L
    precs = a.precs.split(",")
    for p in precs:
        if p not in L.PREC_BY_NAME:
            ap.error(f"unknown precision {p!r}: one of {sorted(L.PREC_BY_NAME)}")
    if not torch.cuda.is_available():
        sys.exit("tools/bench_half_modes.py measures on the GPU; none is visible")
    wl = bench.WORKLOADS[a.workload]
    B = a.batch or wl["batch"]
    lines = [f"# tools/bench_half_modes.py: {a.workload} = {wl['desc']}",
             f"# device {torch.cuda.get_device_name(0)}; batch {B}; {a.warmup} warm-up + {a.steps} timed captured steps per measurement, "
             f"{a.rounds} rounds alternating {' '.join(precs)} in one process"]
    legs = {p: Leg(wl, p, B) for p in precs}
    for leg in legs.values():
        leg.setup()
    ms = {p: [] for p in precs}
    for r in range(a.rounds):
        for p in precs:
            ms[p].append(legs[p].measure(a.steps, a.warmup))
            lines.append(f"round {r + 1} {p:7s} ms_per_step {ms[p][-1]:.3f}")
            print(lines[-1], flush=True)
    base = statistics.median(ms[precs[0]])
    lines.append(f"# mode | median ms/step | spread (max - min) | images/s | vs {precs[0]}")
    for p in precs:
        med, spread = statistics.median(ms[p]), max(ms[p]) - min(ms[p])
        lines.append(f"{a.workload} {p:7s} | {med:8.3f} | {spread:6.3f} | {B / med:8.3f} | {base / med:5.2f}x")
    del legs
    torch.cuda.empty_cache()
    if a.free_run:
        free_run(wl, precs, a.free_run, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
