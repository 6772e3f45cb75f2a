#!/usr/bin/env python3
"""Time of one `clip_scores` call: B pairs of S x S images with their prompts -> the four CLIP scores (synthetic weights).

    python tools/bench_clip_metrics.py [--batch 32] [--size 512] [--clip_model ViT-B/16] [--dtype fp16] [--warmup 3] [--repeats 10]

Prints one JSON line: the median wall time of a call between device synchronisations (after the warm-up calls), and from one further,
instrumented call the share of the device time spent in every entry point of the library (HIP events around each call: the shares, not the
instrumented call's total, are what to read)."""
import argparse
import json
import statistics
import sys
import time
from collections import defaultdict
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "eta-inversion_amd"))


class _Timed:
    """the loaded library with HIP events around every etainv_* call"""

    def __init__(self, lib):
        self._lib, self.events, self.on = lib, [], False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("etainv_") or name in ("etainv_last_error", "etainv_abi_version"):
            return fn

        def call(*args):
            if not self.on:
                return fn(*args)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.events.append((name, a, b))
            return rc
        return call


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--clip_model", default="ViT-B/16")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args(argv)
    from etainv import _capi
    timed = _Timed(_capi.load())
    _capi._lib = timed                                   # before the model is built: its ops keep the handle
    from metrics import ClipModel, clip_scores
    from metrics.clip_similarity import MODES
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = ClipModel("synthetic", "cuda", a.clip_model, compute_dtype=dtype)
    g = torch.Generator().manual_seed(0)
    edit = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    source = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    sp = [f"a photo of a cat number {i} on a bench" for i in range(a.batch)]
    tp = [f"a photo of a dog number {i} on a bench" for i in range(a.batch)]
    names = ["clip_" + m for m in MODES]
    run = lambda: clip_scores(edit, source, sp, tp, names, model)
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    timed.on = True
    run()
    torch.cuda.synchronize()
    timed.on = False
    per = defaultdict(float)
    for name, e0, e1 in timed.events:
        per[name] += e0.elapsed_time(e1)
    total = sum(per.values())
    print(json.dumps({"what": "clip_scores", "batch": a.batch, "size": a.size, "clip_model": a.clip_model, "dtype": a.dtype,
                      "median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
                      "repeats": a.repeats, "warmup": a.warmup, "instrumented_device_ms": round(total, 3),
                      "share": {k: round(v / total, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])},
                      "calls": {k: sum(1 for n, _, _ in timed.events if n == k) for k in per}}))


if __name__ == "__main__":
    main()
