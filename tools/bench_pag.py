#!/usr/bin/env python3
"""Wall clock of DDIM-50 trajectories at C2 (unet_fast ch128, 64x64, bs 40 -> UNet batch 80, f16x3) through
LatentDiffusion.p_sample_loop on the captured step under three guidance forms: CFG (cond_scale 2, the fused step as it is),
perturbed-attention guidance on the middle attention (`pag_scale`, pag_layers 'mid') and on every attention layer ('all').
One process; one untimed run of each first (engines, packed weights, captures), then the three ALTERNATE within each of
`--reps` repetitions, so drift hits all of them alike; synchronised wall clock, best and median kept.

Then, per form, the attention entries of the doubled evaluation's engine launched one by one with a HIP event pair around each
(`_Program.run_profiled`, best of `--profile-reps` passes): the core (`.attn`: QK^T, softmax, PV -- over all 2B samples under
CFG, over the conditional B under PAG) and the value gather of the perturbed half (`.attn_identity`, sgd_attention_identity).

Writes profiles/pag_c2.txt.

    python tools/bench_pag.py [--prec f16x3] [--reps 5] [--scale 1.5] [--out profiles/pag_c2.txt]
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

STEPS = 50


def attention_launches(eng, reps):
    """{tag: best ms} of the attention entries of ``eng``'s program, launched one by one on the buffers of its last evaluation"""
    best = {}
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(reps):
        for tag, _, ms, _, _ in eng.prog.run_profiled(stream):
            if tag.endswith(".attn") or tag.endswith(".attn_identity"):
                best[tag] = min(ms, best.get(tag, float("inf")))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", default="f16x3", choices=["f32", "f16x3", "bf16x3", "f16", "bf16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pag_c2.txt"))
    a = ap.parse_args()
    from sgdm_amd import _lib as L
    from sgdm_amd.diffusion import LatentDiffusion
    wl = bench.WORKLOADS["c2"]
    model, _, data = bench.build_model(wl, "cuda", a.prec)
    diff = LatentDiffusion(device="cuda", **bench.MODEL_PARAMS)
    diff.set_denoise_fn(model.forward, model.forward_with_cond_scale)
    B, S = wl["batch"], wl["image"]
    dkw = dict(cond=data["cond"].cuda(), layout=None, cond_scale=2.0)
    x_T = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(23)).cuda()
    skw = dict(sampling_method="ddim", vis=None, num_timesteps=STEPS, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
               temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True, disable_tqdm=True,
               hip_graph=True)
    layers = model.attention_prefixes()
    variants = [("cfg", {}, None), ("pag-mid", dict(pag_scale=a.scale), ("middle_block.1",)),
                ("pag-all", dict(pag_scale=a.scale, pag_layers="all"), tuple(sorted(layers)))]
    secs = {name: [] for name, _, _ in variants}
    with torch.no_grad():
        for rep in range(a.reps + 1):                   # (the first round is the untimed one: engines, captures)
            for name, opt, _ in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                u8, _ = diff.p_sample_loop("ddim", (B, 3, S, S), dict(skw, **opt), denoise_sample_fn_kwargs=dict(dkw),
                                           condition_kwargs={}, x_T=x_T)
                torch.cuda.synchronize()
                if rep:
                    secs[name].append(time.perf_counter() - t0)
                assert u8.dtype == torch.uint8
    best = {k: min(v) * 1e3 for k, v in secs.items()}
    med = {k: statistics.median(v) * 1e3 for k, v in secs.items()}
    prec = L.PREC_BY_NAME[a.prec]
    key = (2 * B, S, S, prec)
    attn = {}
    with torch.no_grad():
        for name, _, pag in variants:
            eng = model._engines[key if pag is None else key + (("pag",) + pag,)]
            attn[name] = attention_launches(eng, a.profile_reps)
    lines = [f"# tools/bench_pag.py: C2 = {wl['desc'].split(',')[0]}, precision {a.prec}, DDIM-{STEPS}, captured steps, pag_scale {a.scale}",
             f"# device {torch.cuda.get_device_name(0)}; whole p_sample_loop calls (uint8 tail included), synchronised wall clock;",
             f"# the three forms alternate within each of the {a.reps} repetitions (one untimed run of each first)",
             f"# attention layers of the model: {len(layers)} ({', '.join(layers)})",
             f"{'guidance':9s} {'ms/trajectory (best)':>21s} {'median':>9s} {'spread':>7s} {'vs cfg':>8s} {'ms/eval (best)':>15s} "
             f"{'attn core ms/eval':>18s} {'identity ms/eval':>17s}"]
    for name, _, _ in variants:
        core = sum(v for k, v in attn[name].items() if k.endswith(".attn"))
        ident = sum(v for k, v in attn[name].items() if k.endswith(".attn_identity"))
        lines.append(f"{name:9s} {best[name]:21.2f} {med[name]:9.2f} {med[name] / best[name] - 1:7.2%} {best[name] / best['cfg'] - 1:+8.2%} "
                     f"{best[name] / STEPS:15.3f} {core:18.4f} {ident:17.4f}")
    lines.append("# per launch, ms (best of %d event-timed passes; launched one by one, so each includes the launch gap a captured "
                 "step does not pay):" % a.profile_reps)
    lines.append(f"{'entry':34s} " + " ".join(f"{name:>9s}" for name, _, _ in variants))
    tags = sorted({t for v in attn.values() for t in v})
    for t in tags:
        lines.append(f"{t:34s} " + " ".join(f"{attn[name][t]:9.4f}" if t in attn[name] else f"{'-':>9s}" for name, _, _ in variants))
    core_cfg = sum(v for k, v in attn["cfg"].items() if k.endswith(".attn"))
    saved = {name: core_cfg - sum(attn[name].values()) for name, _, _ in variants[1:]}
    lines.append("# attention launches of an evaluation, cfg minus pag (event-timed): "
                 + ", ".join(f"{k} {v:+.4f} ms" for k, v in saved.items())
                 + f"; trajectory best against best per evaluation: "
                 + ", ".join(f"{name} {(best['cfg'] - best[name]) / STEPS:+.4f} ms" for name, _, _ in variants[1:]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
