#!/usr/bin/env python3
"""Cost of learned variance (hparam learn_sigma) at the C2 shape, one process, synthetic data:
  * the training step (forward + backward + AdamW + EMA) of the 6-channel-output model with the hybrid loss
    (sgd_lv_loss_fwd / sgd_lv_loss_bwd) and of the ordinary 3-channel model with the hparam absent, ALTERNATING, so that both
    see the same device state and the same neighbours on the host: best / median / worst over the rounds;
  * the 'native' sampler, captured step: ms per UNet evaluation with the fixed-variance update (sgd_ddpm_step) and with the
    learned-variance one (sgd_ddpm_lv_step);
  * the learned-variance 'native' sampler strided with native_steps = 1000, 250 and 100: seconds per trajectory.
    python tools/bench_learned_variance.py [--batch 40] [--prec f16x3] [--rounds 7] [--steps 5] [--out profiles/learned_variance_c2.txt]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "self-guided-diffusion-models_amd"))
import torch
import bench
from sgdm_amd.diffusion import LatentDiffusion
from sgdm_amd.ema import LitEma
from sgdm_amd.synth import synth_batch, weights_from_seed
from sgdm_amd.unet import UNetModel

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40); ap.add_argument("--prec", default="f16x3")
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--evals", type=int, default=60)
ap.add_argument("--native-steps", default="1000,250,100")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about a step time"
dev = torch.device("cuda", 0)
wl = bench.WORKLOADS["c2"]
S, B = wl["image"], a.batch


def build(out_channels):
    """bench.build_model's C2 model with `out_channels` outputs"""
    m = UNetModel(dropout=0.1, resblock_updown=True, condition=bench.AD(scale_type="imagen"), image_size=S, in_channels=3,
                  out_channels=out_channels, model_channels=wl.get("model_channels", 128), num_res_blocks=2, channel_mult=[1, 2, 4],
                  attention_resolutions=[4], num_heads=8, use_scale_shift_norm=True, cond_dim=wl["cond_dim"],
                  condition_method=wl["method"])
    m.load_state_dict(weights_from_seed([(k, tuple(v.shape)) for k, v in m.state_dict().items()], 23))
    m = m.to(dev)
    m.hip_precision = a.prec
    return m


data = synth_batch(wl["method"], B, S, wl["cond_dim"], wl["layout_dim"], seed=23)
x, cond = data["image"].to(dev), data["cond"].to(dev)
paths = {}
for name, oc, extra in (("default", 3, {}), ("learn_sigma", 6, dict(learn_sigma=True))):
    m = build(oc).train()
    d = LatentDiffusion(device="cuda", **dict(bench.MODEL_PARAMS, **extra)).train()
    d.set_denoise_fn(m.forward, m.forward_with_cond_scale)
    paths[name] = (d, m, torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01), LitEma(m))


def step(name):
    d, m, opt, ema = paths[name]
    loss, _ = d.forward_tao(x, cond=cond, cond_drop_prob=0.1)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    ema(m)
    return loss


for k in paths:
    for _ in range(a.warmup):
        step(k)
ms = {k: [] for k in paths}
for r in range(a.rounds):
    for k in (("default", "learn_sigma") if r % 2 == 0 else ("learn_sigma", "default")):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.steps):
            step(k)
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
lines = [f"C2 training step, bs={B} prec={a.prec} parameterization=eps, {a.rounds} rounds x {a.steps} steps per path, alternating"]
for k, v in ms.items():
    best, med = min(v), statistics.median(v)
    what = "out_channels=6, L_simple + L_vlb" if k == "learn_sigma" else "out_channels=3, hparam absent"
    lines.append(f"{k:11s} ({what}): best {best:.2f} ms  median {med:.2f} ms  worst {max(v):.2f} ms  "
                 f"best-to-median spread {(med - best) / best * 100:.2f} %")
dm = statistics.median(ms["learn_sigma"]) - statistics.median(ms["default"])
lines.append(f"learn_sigma - default: {dm:+.3f} ms on the medians ({dm / statistics.median(ms['default']) * 100:+.2f} %), "
             f"{min(ms['learn_sigma']) - min(ms['default']):+.3f} ms on the bests")

# ---- sampling: the captured 'native' step
skw = dict(sampling_method="native", num_timesteps=1000, ddim_eta=0.0, log_num_per_prog=10, clip_denoised=True, dtp=1,
           temperature=1.0, noise_dropout=0, random_sample_condition=False, return_inter_dict=True)
dkw = dict(cond=cond, layout=None, cond_scale=2.0)
torch.manual_seed(23)
x_T = torch.randn(B, 3, S, S, device=dev)


def sample(name, sk, idx=None):
    d, m, _, _ = paths[name]
    m.eval()
    with torch.no_grad():
        img, _ = d.sampler.sample((B, 3, S, S), sampling_kwargs=sk, denoise_sample_fn=d.denoise_sample_fn,
                                  denoise_sample_fn_kwargs=dkw, x_T=x_T.clone(), **({} if idx is None else dict(step_indices=idx)))
    torch.cuda.synchronize()
    return img


lines.append("")
lines.append(f"'native' sampler, C2, bs={B} (UNet batch {2 * B}), cond_scale=2, captured step, {a.evals} evaluations timed after 5:")
per = {}
for name in paths:
    sample(name, skw, [999])
    sample(name, skw, [999 - i for i in range(5)])
    t0 = time.perf_counter()
    sample(name, skw, [994 - i for i in range(a.evals)])
    per[name] = (time.perf_counter() - t0) / a.evals * 1e3
    upd = "sgd_ddpm_lv_step, 6-wide head" if name == "learn_sigma" else "sgd_ddpm_step, fixed variance"
    lines.append(f"{name:11s} ({upd}): {per[name]:.3f} ms per evaluation")
lines.append("")
lines.append("learn_sigma 'native' trajectories (sampling kwarg native_steps), seconds per trajectory:")
for K in [int(v) for v in a.native_steps.split(",")]:
    sk = dict(skw, native_steps=K)
    sample("learn_sigma", sk, [K - 1])                         # capture outside the timed region
    t0 = time.perf_counter()
    img = sample("learn_sigma", sk)
    dt = time.perf_counter() - t0
    assert torch.isfinite(img).all()
    lines.append(f"native_steps={K:4d}: {dt:.2f} s  ({dt / K * 1e3:.3f} ms per evaluation)")
report = "\n".join(lines)
print(report)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(report + "\n")
