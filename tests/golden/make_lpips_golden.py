"""Writes tests/golden/lpips_ref.npz: the float64 scores of the lpips / bglpips test cases, a subset of their float64 tap values and the yardsticks
of tests/test_lpips_gpu.py.  Run from the repository root:

    python tests/golden/make_lpips_golden.py

The model is the library's synthetic AlexNet-width LPIPS weights (seed 0) and the images come from tests/lpips_ref.make_images(seed): neither is
stored.  Cases (tests/lpips_ref.CASES): 4 pairs at 64 x 64 and 4 pairs at 67 x 70 (the pool's floor drops a row, conv1 leaves columns unread),
each without and with per-pair foreground masks, and one pair at 512 x 512.  Even pairs are a source and the source plus noise 0.1, odd pairs two
independent images.  Per case the file holds
  score_<case>        float64 [pairs]
  tap<l>_<case>       every TAP_STRIDE-th value of tap l as float64 (small cases; tests/test_lpips_ref.py checks that lpips_ref reproduces them, the
                      GPU tests compare against lpips_ref's full tensors)
  y_F_<case>_<l>_<dtype>   max |F_prec - F_64| of tap l, F_prec = lpips_ref's tower with every operand and result rounded to that dtype and fp32
                      arithmetic between two rounding points (dino_ref.Prec), run by torch on the CPU
  y_S_<dtype>         max over the 16 pairs of the four small cases of |s_prec - s_64| / s_64, so that one lucky draw does not set it
Every s_64 exceeds 1e-4 (asserted here and in tests/test_lpips_ref.py), so the ratio is well conditioned."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "eta-inversion_amd")]
from tests import lpips_ref as lr  # noqa: E402
from tests.dino_ref import Prec  # noqa: E402

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def main():
    sd = lr.model_state_dict()
    out, y_s = {}, {name: 0.0 for name in DTYPES}
    for case in lr.CASES:
        x, b, mask = lr.case_inputs(case)
        s64, t64 = lr.score(sd, x, b, -1, 1, mask)
        assert s64.min() > 1e-4, (case, s64)
        out[f"score_{case}"] = s64.numpy()
        print(f"{case}: scores {[round(v, 6) for v in s64.tolist()]} taps {[tuple(t.shape[1:]) for t in t64]}")
        if case not in lr.SMALL:
            continue
        for l, t in enumerate(t64):
            out[f"tap{l}_{case}"] = t.flatten()[::lr.TAP_STRIDE].numpy()
        for name, dt in DTYPES.items():
            sp, tp = lr.score(sd, x, b, -1, 1, mask, Prec(dt))
            y_s[name] = max(y_s[name], ((sp - s64).abs() / s64).max().item())
            for l, (a, c) in enumerate(zip(tp, t64)):
                out[f"y_F_{case}_{l}_{name}"] = np.float64((a - c).abs().max().item())
            print(f"  {name}: y_F {[float(out[f'y_F_{case}_{l}_{name}']) for l in range(5)]}")
    for name, y in y_s.items():
        out[f"y_S_{name}"] = np.float64(y)
        print(f"y_S {name}: {y:.3e}")
    path = ROOT / "tests" / "golden" / "lpips_ref.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
