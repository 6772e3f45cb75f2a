#!/usr/bin/env python3
"""Time etainv_prox_guidance (csrc/proximal.hip) against the chain of eager torch launches it replaces, on the GPU.

    python tools/bench_prox_guidance.py [--rounds 200] [--e2e]

Per size (l, rows per group): device-event time per call of (a) the fused launch with the DDIM step, l0 at quantile 0.7, (b) the same in
pass-through mode, (c) the reference's lines in eager torch on the device -- the subtraction, abs, torch.quantile, clamp, the guided noise and
the DDIM step --, the three alternated round by round in one process; prints median and minimum in microseconds and one JSON line.
--e2e adds the backward pass of a proxnpi [source, target] edit at L = 64 (S = 50, fp16), host clock around a synchronised pass, through the
fused path and through the per-step path, twice each, alternated."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "eta-inversion_amd"):
    sys.path.insert(0, str(p))

SIZES = [(8, 2), (16, 2), (20, 2), (44, 3), (64, 2), (64, 4), (96, 2), (96, 4)]
G, Q, A_FROM, A_TO = 7.5, 0.7, 0.8, 0.9


def eager(u, c, x):
    d = c - u
    thr = d.abs().quantile(Q)
    d = d - d.clamp(-thr, thr)
    eps = u + G * d
    x0 = (x - (1 - A_FROM) ** 0.5 * eps) / A_FROM ** 0.5
    return A_TO ** 0.5 * x0 + (1 - A_TO) ** 0.5 * eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from etainv import _capi
    from etainv.pipeline import ProximalGuidance
    lib, result = _capi.load(), {}
    for l, rows in SIZES:
        gen = torch.Generator().manual_seed(l)
        u, c, x = (torch.randn(rows, 4, l, l, generator=gen).cuda() for _ in range(3))
        out, x_out = torch.empty_like(c), torch.empty_like(x)
        prox, plain = ProximalGuidance(l, "l0", Q), ProximalGuidance(l, None)
        arms = {"fused_l0": lambda: prox.run(lib, u, c, G, out, x, A_FROM, A_TO, x_out, 1, rows),
                "fused_plain": lambda: plain.run(lib, u, c, G, out, x, A_FROM, A_TO, x_out, 1, rows),
                "eager_torch": lambda: eager(u, c, x)}
        want = eager(u, c, x)
        arms["fused_l0"]()
        assert (x_out - want).abs().max() < 1e-4                                       # the three arms compute the same thing
        times = {k: [] for k in arms}
        for r in range(a.rounds + 20):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= 20:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        result[f"{l}x{rows}"] = {k: (float(np.median(v)), float(np.min(v))) for k, v in times.items()}
        print(f"l = {l:2d} rows = {rows} ({rows * 4 * l * l:6d} values): " +
              ", ".join(f"{k} median {np.median(v):7.1f} us (min {np.min(v):7.1f})" for k, v in times.items()))
    if a.e2e:
        import modules
        L, S = 64, 50
        p = modules.load_diffusion_model("sd15", "cuda", variant="fp16", latent_size=L, max_img=1)[0]
        inv = modules.load_inverter("proxnpi", model=p, scheduler="ddim", num_inference_steps=S)
        gen = torch.Generator().manual_seed(1)
        z0 = 0.8 * torch.randn(1, 4, L, L, generator=gen).cuda()
        ctx_s, ctx_t = torch.randn(2, 77, 768, generator=gen).cuda(), torch.randn(2, 77, 768, generator=gen).cuda()
        inv.encode = lambda image: image
        res = inv.invert(z0, context=ctx_s)
        for per_step in (False, True, False, True):
            inv.force_per_step = per_step
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lat = inv.diffusion_backward(torch.cat([res["latents"][-1]] * 2), inv.cat_context([ctx_s, ctx_t]), res)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            result.setdefault("e2e_backward_s", {}).setdefault("per_step" if per_step else "fused", []).append(dt)
            print(f"proxnpi backward pass, S = {S}, L = {L}, fp16, {'per-step' if per_step else 'fused'} path: {dt:.3f} s ({dt / S * 1e3:.2f} ms per step)")
        assert torch.isfinite(lat).all()
        p.engine.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
