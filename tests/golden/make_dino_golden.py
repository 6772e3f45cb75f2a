"""Writes tests/golden/dino_ref.npz: the float64 keys and scores of the dinovitstruct test cases, the yardsticks of tests/test_dino_gpu.py, and
values recorded from the reference's own code.  Run from the repository root:

    python tests/golden/make_dino_golden.py --reference <checkout of the reference project>

The models are drawn from seeds (tests/dino_ref.random_state_dict: int8 times a power of two, exact in fp16 and bf16), so no weight is stored:
  case A   width 128 (2 heads), 3 layers, patch 8, image 32 (17 tokens); 8 pairs at S = 20 (upscale) and 8 pairs at S = 64
  case B   width 128, 2 layers, patch 8, image 224 (785 tokens); 2 pairs at S = 256
  syn      the library's synthetic weights at the "tiny/8" geometry, on case A's S = 20 pairs
Images come from dino_ref.make_images(seed) and are not stored.  Per case the file holds the float64 scores of every pair, the float64 keys at
every `stride`-th token (the full key tensors would not fit the repository's size limit; tests/test_dino_ref.py checks that dino_ref reproduces
what is stored, the GPU tests compare against dino_ref's full tensors), and per dtype
  y_K      max |K_prec - K_64|, K_prec = dino_ref's tower with every operand and result rounded to that dtype (dino_ref.Prec), run by torch on the CPU
  y_S      max over the case's pairs of |s_prec - s_64| / s_64, s_prec = the score of K_prec; for case A over the 16 pairs of both sizes
Every pair's s_64 exceeds 1e-3 (asserted here), so the ratio is well conditioned.

From the reference (imported at generation time only; nothing of it is stored but numbers):
  ref_sim, ref_mse   `attn_cosine_sim` and `F.mse_loss` of metrics/dino_vit_structure.py on case A's S = 20 float64 keys, pair by pair, and on a
                     copy of pair 0 whose source keys have one all-zero row
  ref_e2e            `DinoVitStructure.forward` on one pair at S = 240, driven through its `VitExtractor` with `torch.hub.load` replaced by a small
                     module of our own (below: DINO's forward pass with `blocks[i].attn.{qkv, attn_drop}` to hook) holding a seeded 12-block,
                     width-384 model ("dino_vits8": the reference asserts 12 blocks and reads width and heads off the name).
torchvision is not installed where this runs, and the reference imports `Resize`, `Normalize` and `Compose` from it: stand-ins are placed in
sys.modules.  `Resize(224, max_size=480)` on a square float tensor is F.interpolate(mode="bilinear", align_corners=False, antialias=True) to
224 x 224, and that call is the stand-in; Normalize and Compose are the obvious two lines each."""
import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "eta-inversion_amd")]
from tests import dino_ref as dr  # noqa: E402

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
CASES, E2E = dr.CASES, dr.E2E


# ---------------------------------------------------------------------------------------------------------------- what stands in for torch.hub
class _Attn(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.qkv, self.proj, self.attn_drop, self.heads = nn.Linear(d, 3 * d), nn.Linear(d, d), nn.Identity(), d // 64

    def forward(self, x):
        b, n, c = x.shape
        q, k, v = self.qkv(x).reshape(b, n, 3, self.heads, c // self.heads).permute(2, 0, 3, 1, 4)
        a = self.attn_drop((q @ k.transpose(-1, -2) * (c // self.heads) ** -0.5).softmax(-1))
        return self.proj((a @ v).transpose(1, 2).reshape(b, n, c)), a


class _Mlp(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.norm1, self.attn, self.norm2, self.mlp = nn.LayerNorm(d, eps=1e-6), _Attn(d), nn.LayerNorm(d, eps=1e-6), _Mlp(d)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))[0]
        return x + self.mlp(self.norm2(x))


class _PatchEmbed(nn.Module):
    def __init__(self, d, p):
        super().__init__()
        self.proj = nn.Conv2d(3, d, p, stride=p)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class StandInDino(nn.Module):
    def __init__(self, sd):
        super().__init__()
        gm = dr.geometry(sd)
        d = gm["width"]
        self.patch_embed = _PatchEmbed(d, gm["patch"])
        self.cls_token, self.pos_embed = nn.Parameter(torch.zeros(1, 1, d)), nn.Parameter(torch.zeros(1, sd["pos_embed"].shape[1], d))
        self.blocks = nn.ModuleList([_Block(d) for _ in range(gm["layers"])])
        self.norm = nn.LayerNorm(d, eps=1e-6)
        self.load_state_dict(sd, strict=True)
        self.double()

    def forward(self, x):
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], 1) + self.pos_embed
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)[:, 0]


def load_reference(ref: Path, hub_model):
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

    class Resize:
        def __init__(self, size, max_size=None):
            self.size = size

        def __call__(self, x):
            assert x.dim() == 3 and x.shape[-1] == x.shape[-2]
            return F.interpolate(x[None], size=(self.size, self.size), mode="bilinear", align_corners=False, antialias=True)[0]

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, x):
            return (x - torch.tensor(self.mean, dtype=x.dtype).view(3, 1, 1)) / torch.tensor(self.std, dtype=x.dtype).view(3, 1, 1)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    tr.Resize, tr.Normalize, tr.Compose, tv.transforms = Resize, Normalize, Compose, tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    pkg = types.ModuleType("refmetrics")
    pkg.__path__ = [str(ref / "metrics")]
    sys.modules["refmetrics"] = pkg
    mods = {}
    for name in ("base", "dino_vit_structure"):
        spec = importlib.util.spec_from_file_location(f"refmetrics.{name}", ref / "metrics" / f"{name}.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"refmetrics.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    torch.hub.load = lambda repo, name: hub_model
    return mods["dino_vit_structure"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    out, k64, s64, kp, sp = {}, {}, {}, {}, {}
    for case, c in CASES.items():
        sd, x, b = dr.case_inputs(case)
        k64[case] = dr.image_keys(sd, x, -1, 1)
        s64[case] = dr.score(k64[case][:b], k64[case][b:])
        assert s64[case].min() > 1e-3, (case, s64[case])
        out[f"keys_{case}"], out[f"stride_{case}"], out[f"score_{case}"] = k64[case][:, ::c["stride"]].numpy(), np.int32(c["stride"]), s64[case].numpy()
        print(f"{case}: keys {tuple(k64[case].shape)} |K| max {k64[case].abs().max():.3f} scores {[round(v, 5) for v in s64[case].tolist()]}")
        for name, dt in DTYPES.items():
            k = dr.image_keys(sd, x, -1, 1, dr.Prec(dt))
            kp[case, name], sp[case, name] = (k - k64[case]).abs().max().item(), ((dr.score(k[:b], k[b:]) - s64[case]).abs() / s64[case]).max().item()
    for name in DTYPES:
        for case in CASES:
            out[f"y_K_{case}_{name}"] = np.float64(kp[case, name])
        ya = max(sp["a20", name], sp["a64", name])
        for case, y in (("a20", ya), ("a64", ya), ("b", sp["b", name]), ("syn", sp["syn", name])):
            out[f"y_S_{case}_{name}"] = np.float64(y)
            print(f"y {case} {name}: keys {kp[case, name]:.3e} score {y:.3e}")

    # the reference's own self-similarity and loss on case A's keys, and on keys with an all-zero row
    sd_e = dr.random_state_dict(**{k: E2E[k] for k in ("width", "layers", "patch", "image", "seed")})
    ref = load_reference(Path(a.reference), StandInDino(sd_e))
    ka = k64["a20"]
    zero = ka[[0, 8]].clone()
    zero[0, 5] = 0.0
    pairs = [(ka[i], ka[8 + i]) for i in range(8)] + [(zero[0], zero[1])]
    sims = torch.stack([torch.stack([ref.attn_cosine_sim(k[None, None])[0] for k in p]) for p in pairs])            # [9][2][17][17]
    mse = torch.stack([F.mse_loss(s[1], s[0]) for s in sims])
    assert torch.isfinite(sims).all() and (sims[8, 0, 5] == 0).all()
    assert (dr.self_sim(torch.stack([p[0] for p in pairs])) - sims[:, 0]).abs().max() < 1e-12
    assert (dr.score(torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])) - mse).abs().max() < 1e-12
    out["ref_sim"], out["ref_mse"], out["ref_zero_row"] = sims.numpy(), mse.numpy(), np.int32(5)
    # ... and its metric class end to end on the stand-in model
    src, edit = dr.make_images(1, E2E["s"], -1, 1, E2E["image_seed"])
    metric = ref.DinoVitStructure(input_range=(-1, 1), device="cpu", vit_model="dino_vits8")
    with torch.no_grad():
        e2e = float(metric.forward(edit.double(), src.double()))
        ke = dr.image_keys(sd_e, torch.cat([src, edit]), -1, 1)
    ours = float(dr.score(ke[:1], ke[1:])[0])
    print(f"reference class end to end: {e2e:.12g}, dino_ref {ours:.12g}, |diff| {abs(e2e - ours):.3e}")
    assert abs(e2e - ours) < 1e-10 * max(e2e, 1e-3) and repr(metric) == "dino_vits8"
    out["ref_e2e"] = np.float64(e2e)
    path = ROOT / "tests" / "golden" / "dino_ref.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
