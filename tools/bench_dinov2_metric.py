#!/usr/bin/env python3
"""Time of one `dino_structure` call on a DINOv2 model (dinovitstruct_v2): B pairs of S x S images -> B structure distances (synthetic weights).

    python tools/bench_dinov2_metric.py [--batch 8] [--size 512] [--dino_model dinov2_vitb14] [--dtype fp16] [--warmup 3] [--repeats 10]

Prints one JSON line:
  median_ms     the median wall time of a call between device synchronisations, after the warm-up calls
  device_ms     the median device time of its three parts (preprocess, tower, self-similarity), each between torch events
  kernels_ms    the tower again with an event pair around every C-ABI call, summed per entry point over one pass and the median taken over the
                repeats (each event pair adds a few microseconds of its own, so the sum exceeds `tower`; read the shares)
  fused_vs_unfused  etainv_op_layerscale_add_layernorm at rows = B tokens (2056 at the defaults) and the model's width beside the pair it replaces:
                torch.addcmul(x, gamma, y) into a new tensor plus etainv_op_layernorm of that tensor.  The two are timed alternately, `inner`
                launches per event pair; median microseconds per launch (per pair of launches for the unfused form), and the bytes each must
                move over that time.  Both read and write the same bits of h; the unfused pair rounds gamma to the compute type, which the
                fused kernel does not."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "eta-inversion_amd"))


class _TimedLib:
    """stands in for the ctypes library of a tower's `_Ops`: every etainv_* call between two events"""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("etainv_op") and not name.startswith("etainv_clip") and not name.startswith("etainv_dino"):
            return fn

        def call(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.log.append((name, a, b))
            return rc
        return call


def _fused_vs_unfused(rows, c, dtype, repeats, inner=20):
    from etainv import _capi
    lib = _capi.load()
    g = torch.Generator().manual_seed(1)
    x, y = (torch.randn(rows, c, generator=g).to(dtype).cuda() for _ in range(2))
    ls = torch.pow(10.0, -5.0 * torch.rand(c, generator=g)).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).cuda(), (0.1 * torch.randn(c, generator=g)).cuda()
    ls_t, code = ls.to(dtype), _capi.dtype_code(dtype)
    xo, h = torch.empty_like(x), torch.empty_like(x)

    def fused():
        _capi.check(lib.etainv_op_layerscale_add_layernorm(_capi.ptr(y), _capi.ptr(ls), _capi.ptr(x), _capi.ptr(gamma), _capi.ptr(beta), 1e-6, _capi.ptr(xo),
                                                           _capi.ptr(h), rows, c, code, _capi.stream_ptr()))

    def unfused():
        t = torch.addcmul(x, ls_t, y)
        _capi.check(lib.etainv_op_layernorm(_capi.ptr(t), _capi.ptr(gamma), _capi.ptr(beta), _capi.ptr(h), rows, c, 1e-6, code, _capi.stream_ptr()))

    times = {"fused": [], "unfused": []}
    for rep in range(repeats + 2):
        for name, fn in (("fused", fused), ("unfused", unfused)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append(a.elapsed_time(b) * 1e3 / inner)
    es = x.element_size()
    moved = {"fused": 4 * rows * c * es, "unfused": 6 * rows * c * es}            # y, x in, x_out, h out; the pair reads x_out back and writes it twice over
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"rows": rows, "c": c, "inner": inner, "us": {k: round(v, 2) for k, v in med.items()},
            "min_us": {k: round(min(v), 2) for k, v in times.items()}, "gb_per_s": {k: round(moved[k] / med[k] / 1e3, 1) for k in med},
            "unfused_over_fused": round(med["unfused"] / med["fused"], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dino_model", default="dinov2_vitb14")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args(argv)
    from metrics import Dinov2Model, dino_structure
    from metrics.dino_vit_structure import dinov2_preprocess, key_self_similarity_mse
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    model = Dinov2Model("synthetic", "cuda", a.dino_model, compute_dtype=dtype)
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
        rows = dinov2_preprocess(both, (-1, 1), model.image, dtype, model.antialias)
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
    ops = model.backend.ops
    plain, per_call, counts = ops.lib, {}, {}
    for _ in range(a.repeats):
        ops.lib = timed = _TimedLib(plain)
        model.backend(rows, 2 * a.batch)
        torch.cuda.synchronize()
        ops.lib = plain
        sums = {}
        for name, e0, e1 in timed.log:
            sums[name] = sums.get(name, 0.0) + e0.elapsed_time(e1)
            counts[name] = counts.get(name, 0) + 1
        for name, v in sums.items():
            per_call.setdefault(name, []).append(v)
    kernels = {k: round(statistics.median(v), 3) for k, v in per_call.items()}
    n = model.backend.g2 + 1
    print(json.dumps({"what": "dino_structure (dinov2)", "batch": a.batch, "size": a.size, "dino_model": a.dino_model, "dtype": a.dtype,
                      "tokens": n, "width": model.width, "median_ms": round(statistics.median(wall), 3),
                      "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3), "repeats": a.repeats, "warmup": a.warmup,
                      "device_ms": {k: round(v, 3) for k, v in med.items()}, "share": {k: round(v / total, 4) for k, v in med.items()},
                      "kernels_ms": kernels, "launches": {k: v // a.repeats for k, v in counts.items()},
                      "fused_vs_unfused": _fused_vs_unfused(a.batch * n, model.width, dtype, a.repeats) if dtype != torch.float32 or model.width <= 1280
                      else None, "score_mean": float(scores.mean())}))


if __name__ == "__main__":
    main()
