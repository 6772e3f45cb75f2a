#!/usr/bin/env python3
"""Time of one `lpips_distance` call: B pairs of S x S images -> B LPIPS distances (synthetic AlexNet-width weights), kernel by kernel.

    python tools/bench_lpips_metric.py [--batch 32] [--size 512] [--dtype fp16] [--warmup 3] [--repeats 10] [--no_torch]

Prints one JSON line: the median wall time of a call between device synchronisations (after the warm-up calls) and, between torch events over
the same repeats, the median device time of every launch of the call: the preprocess, the five convolutions (with their algorithmic
2 M N K FLOPs as TFLOP/s and as a share of the MFMA peak of the dtype: 2512 TFLOP/s for fp16 / bf16, 157 for fp32 operands), the two poolings and
the five distance calls (with the bytes they must move -- input read once, output written once -- as GB/s and as a share of 8 TB/s of HBM).
Unless --no_torch: the same five convolutions + ReLU and two poolings through torch's F.conv2d / F.max_pool2d on the same device, dtype and
values (NCHW, torch's default layout; its own warm-up, so that the library's kernel search is outside the timing), layer by layer."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "eta-inversion_amd"))
MFMA_PEAK = {"fp16": 2512e12, "bf16": 2512e12, "fp32": 157e12}
HBM_PEAK = 8e12


def _timed(steps, repeats):
    """steps: [(name, callable)] run in order -> {name: median device ms}"""
    times = {name: [] for name, _ in steps}
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record()
        for i, (_, fn) in enumerate(steps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(steps):
            times[name].append(ev[i].elapsed_time(ev[i + 1]))
    return {k: statistics.median(v) for k, v in times.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no_torch", action="store_true")
    a = ap.parse_args(argv)
    from etainv.weights import LPIPS_CONVS, LPIPS_KERNELS, synthetic_lpips_state_dict
    from metrics import LpipsModel, lpips_distance
    from metrics.lpips import layer_distance, lpips_preprocess
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    esize = 4 if a.dtype == "fp32" else 2
    model = LpipsModel("synthetic", "cuda", compute_dtype=dtype)
    net, n, s = model.backend, 2 * a.batch, a.size
    g = torch.Generator().manual_seed(0)
    source = (torch.rand(a.batch, 3, s, s, generator=g) * 2 - 1).cuda()
    edit = (source + 0.1 * torch.randn(a.batch, 3, s, s, generator=g).cuda()).clamp(-1, 1)
    both = torch.cat([source, edit])
    for _ in range(a.warmup):
        scores = lpips_distance(edit, source, model)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        lpips_distance(edit, source, model)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)

    sizes, wd = net.tap_sizes(s, s), net.widths
    taps, p1, p2 = net._buffers[(n, s, s, str(both.device))]
    state = {}
    out = torch.zeros(a.batch, dtype=torch.float64, device="cuda")
    steps = [("preprocess", lambda: state.update(x=lpips_preprocess(both, (-1, 1), None, dtype))),
             ("conv1", lambda: net._conv(state["x"], taps[0], n, s, s, 0)), ("pool1", lambda: net._pool(taps[0], p1, n, *sizes[0], wd[0])),
             ("conv2", lambda: net._conv(p1, taps[1], n, *sizes[1], 1)), ("pool2", lambda: net._pool(taps[1], p2, n, *sizes[1], wd[1])),
             ("conv3", lambda: net._conv(p2, taps[2], n, *sizes[2], 2)), ("conv4", lambda: net._conv(taps[2], taps[3], n, *sizes[2], 3)),
             ("conv5", lambda: net._conv(taps[3], taps[4], n, *sizes[2], 4))]
    steps += [(f"distance{l + 1}", (lambda l=l: layer_distance(taps[l], net.lins[l], out))) for l in range(5)]
    med = _timed(steps, a.repeats)
    px = lambda hw: hw[0] * hw[1]
    cins = (3,) + wd[:4]
    kernels = {"preprocess": {"ms": med["preprocess"], "bytes": n * s * s * (12 + 4 * esize)}}
    for l in range(5):
        k = LPIPS_KERNELS[l][0]
        flops = 2.0 * n * px(sizes[l]) * wd[l] * k * k * cins[l]
        kernels[f"conv{l + 1}"] = {"ms": med[f"conv{l + 1}"], "gflop": flops / 1e9, "tflops": flops / med[f"conv{l + 1}"] / 1e9,
                                   "of_mfma_peak": flops / med[f"conv{l + 1}"] / 1e-3 / MFMA_PEAK[a.dtype]}
        kernels[f"distance{l + 1}"] = {"ms": med[f"distance{l + 1}"], "bytes": n * px(sizes[l]) * wd[l] * esize}
    for i, l in ((1, 0), (2, 1)):
        kernels[f"pool{i}"] = {"ms": med[f"pool{i}"], "bytes": n * (px(sizes[l]) + px(sizes[l + 1])) * wd[l] * esize}
    for v in kernels.values():
        if "bytes" in v:
            v["gbs"] = v["bytes"] / v["ms"] / 1e6
            v["of_hbm_peak"] = v["bytes"] / v["ms"] / 1e-3 / HBM_PEAK
    res = {"what": "lpips_distance", "batch": a.batch, "size": s, "dtype": a.dtype, "median_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3),
           "max_ms": round(max(wall), 3), "repeats": a.repeats, "warmup": a.warmup, "device_ms_sum": round(sum(med.values()), 3),
           "kernels": {k: {kk: round(vv, 4) for kk, vv in v.items()} for k, v in kernels.items()}, "score_mean": float(scores.mean())}

    if not a.no_torch:
        sd = synthetic_lpips_state_dict()
        ws = [(sd[f"features.{c}.weight"].to("cuda", dtype), sd[f"features.{c}.bias"].to("cuda", dtype)) + LPIPS_KERNELS[i][1:] for i, c in enumerate(LPIPS_CONVS)]
        tstate = {"x0": state["x"][..., :3].permute(0, 3, 1, 2).contiguous()}
        conv = lambda i, src, dst: (lambda: tstate.update({dst: F.relu(F.conv2d(tstate[src], ws[i][0], ws[i][1], stride=ws[i][2], padding=ws[i][3]))}))
        pool = lambda src, dst: (lambda: tstate.update({dst: F.max_pool2d(tstate[src], 3, 2)}))
        tsteps = [("conv1", conv(0, "x0", "t1")), ("pool1", pool("t1", "p1")), ("conv2", conv(1, "p1", "t2")), ("pool2", pool("t2", "p2")),
                  ("conv3", conv(2, "p2", "t3")), ("conv4", conv(3, "t3", "t4")), ("conv5", conv(4, "t4", "t5"))]
        for _ in range(max(a.warmup, 2)):
            for _, fn in tsteps:
                fn()
        torch.cuda.synchronize()
        tmed = _timed(tsteps, a.repeats)
        err = float((tstate["t5"].permute(0, 2, 3, 1).reshape(n, -1, wd[4]).float() - taps[4].float()).abs().max())
        res["torch_ms"] = {k: round(v, 4) for k, v in tmed.items()}
        res["torch_over_native"] = {k: round(tmed[k] / med[k], 3) for k in tmed}
        res["torch_tap5_max_abs_diff"] = err
    print(json.dumps(res))


if __name__ == "__main__":
    main()
