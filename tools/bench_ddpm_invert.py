#!/usr/bin/env python3
"""Wall time of the `ddpminv` inversion, time-parallel against per-step ("DDPM inversion"; for information, no threshold).

    python tools/bench_ddpm_invert.py [--steps 50] [--latent 64] [--rows 128] [--prec fp16] [--repeats 5]

One image, the default forward guidance 3.5 (both halves of every step run).  The time-parallel path sends the S steps to the UNet in chunks of
rows // 2 steps and follows each with one etainv_ddpm_invert_steps launch; `force_per_step` is the reference's loop, one 2-row UNet call and one
k = 1 launch per step.  Both are timed with a host clock around work that ends in a device synchronise, after a warm-up of each, alternating,
on one engine with synthetic weights; the UNet calls of each are counted.  Prints one JSON line."""
import argparse
import json
import sys
import time
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "eta-inversion_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--prec", default="fp16", choices=("fp16", "bf16", "fp32"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from etainv.engine import Engine
    from modules.inversion.ddpm_inversion import DDPMInversion
    from modules.models import NativeUNet
    from modules.schedulers import DDIMScheduler
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.prec]
    engine = Engine(dtype=dtype, max_unet_batch=a.rows, latent_size=a.latent, max_img=1)
    engine.load_synthetic(0)
    model = types.SimpleNamespace(engine=engine, unet=NativeUNet(engine, torch.float32), device=engine.device,
                                  scheduler=DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                                                          set_alpha_to_one=False))
    inv = DDPMInversion(model, num_inference_steps=a.steps)
    g = torch.Generator().manual_seed(0)
    z0 = (0.8 * torch.randn(1, 4, a.latent, a.latent, generator=g)).cuda()
    ctx = torch.randn(2, 77, 768, generator=g).cuda()
    calls, orig = [], engine.unet

    def counted(latent, t, c, ctrl=None, out=None):
        calls.append(c.shape[0])
        return orig(latent, t, c, ctrl, out=out)
    engine.unet = counted

    def run(per_step):
        inv.force_per_step = per_step
        calls.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = inv.diffusion_forward(z0, ctx)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, list(calls), res

    _, _, fast = run(False)                                            # warm-up of every shape either path uses
    _, _, slow = run(True)
    rel = lambda x, y: ((torch.stack(x) - torch.stack(y)).norm() / torch.stack(y).norm()).item()
    times = {False: [], True: []}
    for _ in range(a.repeats):
        for per_step in (False, True):
            dt, n, _ = run(per_step)
            times[per_step].append(dt)
            rows = n
            if per_step:
                calls_slow = rows
            else:
                calls_fast = rows
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"what": "ddpminv diffusion_forward wall time", "steps": a.steps, "latent": a.latent, "engine_rows": a.rows, "prec": a.prec,
                      "time_parallel_s": {"median": med(times[False]), "min": min(times[False]), "max": max(times[False])},
                      "per_step_s": {"median": med(times[True]), "min": min(times[True]), "max": max(times[True])},
                      "unet_calls": {"time_parallel": len(calls_fast), "per_step": len(calls_slow)},
                      "unet_rows_per_call": {"time_parallel": sorted(set(calls_fast)), "per_step": sorted(set(calls_slow))},
                      "speedup_median": med(times[True]) / med(times[False]),
                      "noise_preds_rel_l2_between_paths": rel(fast["noise_preds"], slow["noise_preds"])}))
    engine.close()


if __name__ == "__main__":
    main()
