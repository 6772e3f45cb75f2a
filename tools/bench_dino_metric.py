#!/usr/bin/env python3
"""Time of one `dino_structure` call: B pairs of S x S images -> B structure distances (synthetic weights).

    python tools/bench_dino_metric.py [--batch 8] [--size 512] [--dino_model dino_vitb8] [--dtype fp16] [--warmup 3] [--repeats 10]

Prints one JSON line: the median wall time of a call between device synchronisations (after the warm-up calls), and the median device time of its
three parts -- preprocess (one launch for the 2 B images), tower (one pass over the 2 B images up to the last block's keys) and self-similarity
(one etainv_dino_selfsim_mse call) -- each between torch events, over the same repeats.  By arithmetic the ViT-B/8 tower is about 155 GFLOP per
image and the self-similarity under 2 GFLOP per pair: the number to read is the tower's share."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "eta-inversion_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dino_model", default="dino_vitb8")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args(argv)
    from metrics import DinoModel, dino_structure
    from metrics.dino_vit_structure import dino_preprocess, key_self_similarity_mse
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = DinoModel("synthetic", "cuda", a.dino_model, compute_dtype=dtype)
    g = torch.Generator().manual_seed(0)
    source = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    edit = (source + 0.2 * torch.randn(a.batch, 3, a.size, a.size, generator=g).cuda()).clamp(-1, 1)
    both = torch.cat([source, edit])
    for _ in range(a.warmup):
        dino_structure(edit, source, model)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dino_structure(edit, source, model)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    parts = {"preprocess": [], "tower": [], "selfsim": []}
    for _ in range(a.repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        rows = dino_preprocess(both, (-1, 1), model.image, model.patch, dtype, model.antialias)
        ev[1].record()
        keys = model.backend(rows, 2 * a.batch)
        ev[2].record()
        scores = key_self_similarity_mse(keys)
        ev[3].record()
        torch.cuda.synchronize()
        for name, i in (("preprocess", 0), ("tower", 1), ("selfsim", 2)):
            parts[name].append(ev[i].elapsed_time(ev[i + 1]))
    med = {k: statistics.median(v) for k, v in parts.items()}
    total = sum(med.values())
    print(json.dumps({"what": "dino_structure", "batch": a.batch, "size": a.size, "dino_model": a.dino_model, "dtype": a.dtype,
                      "tokens": model.backend.g2 + 1, "width": model.width, "median_ms": round(statistics.median(wall), 3),
                      "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3), "repeats": a.repeats, "warmup": a.warmup,
                      "device_ms": {k: round(v, 3) for k, v in med.items()}, "share": {k: round(v / total, 4) for k, v in med.items()},
                      "score_mean": float(scores.mean())}))


if __name__ == "__main__":
    main()
