"""Writes tests/golden/dinov2_ref.npz: the float64 keys and scores of the dinovitstruct_v2 test cases, the yardsticks of tests/test_dinov2_gpu.py,
and values recorded from the reference's own code.  Run from the repository root:

    python tests/golden/make_dinov2_golden.py --reference <checkout of the reference project>

The models are drawn from seeds (tests/dinov2_ref.random_state_dict: int8 times a power of two, LayerScale gammas powers of two), no weight is stored:
  case A   width 128 (2 heads), 3 layers, image 42, position table 5 x 5 interpolated to 3 x 3 (10 tokens); 8 pairs at S = 20 and 8 at S = 64
  case B   width 128, 2 layers, image 224, table 37 x 37 interpolated to 16 x 16 (257 tokens: one past four 64-wide tiles); 2 pairs at S = 256
  syn      the library's synthetic weights at the "tinyv2/14" geometry, on case A's S = 20 pairs
Images come from dino_ref.make_images(seed).  Per case the file holds the float64 scores of every pair, the float64 keys at every `stride`-th token
and per dtype the yardsticks y_K and y_S, defined as in tests/golden/make_dino_golden.py (dino_ref.Prec run by torch on the CPU; y_S of case A
over the 16 pairs of both sizes).  Every pair's s_64 exceeds 1e-3 (asserted here).

From the reference (imported at generation time only; nothing of it is stored but numbers):
  ref_e2e     `DinoVitStructure.forward` with vit_model="dinov2_vits14" on one pair at S = 240, driven through its `VitExtractor` with
              `torch.hub.load` replaced by a small module of our own (below) holding a seeded 12-block, width-384 DINOv2-shaped model: patch 14,
              LayerScale, and `interpolate_pos_encoding` as the published hub code states it (F.interpolate, bicubic, scale_factor
              (g + 0.1) / M) -- so the recorded value also pins dinov2_ref's bicubic restatement against torch's own kernel in float64
  ref_keys    the keys its `VitExtractor.get_keys_from_input(layer_num=11)` returns for the source image, heads concatenated, every 16th token
The torchvision stand-ins are those of make_dino_golden.py."""
import argparse
import math
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "eta-inversion_amd")]
from tests import dinov2_ref as v2  # noqa: E402
from tests.golden.make_dino_golden import DTYPES, _Attn, _Mlp, _PatchEmbed, load_reference  # noqa: E402


class _LayerScale(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(d))

    def forward(self, x):
        return x * self.gamma


class _Block(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(d, eps=1e-6), _Attn(d), _LayerScale(d)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(d, eps=1e-6), _Mlp(d), _LayerScale(d)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x))[0])
        return x + self.ls2(self.mlp(self.norm2(x)))


class StandInDinov2(nn.Module):
    """DINOv2's forward pass with `blocks[i].attn.{qkv, attn_drop}` to hook, float64"""
    interpolate_offset = 0.1

    def __init__(self, sd):
        super().__init__()
        gm = v2.geometry(sd)
        d = gm["width"]
        self.patch_embed = _PatchEmbed(d, 14)
        self.cls_token, self.pos_embed = nn.Parameter(torch.zeros(1, 1, d)), nn.Parameter(torch.zeros(1, sd["pos_embed"].shape[1], d))
        self.mask_token = nn.Parameter(torch.zeros(1, d))
        self.blocks = nn.ModuleList([_Block(d) for _ in range(gm["layers"])])
        self.norm = nn.LayerNorm(d, eps=1e-6)
        self.load_state_dict(sd, strict=True)
        self.double()

    def interpolate_pos_encoding(self, x, w, h):
        n_patch, n_pos = x.shape[1] - 1, self.pos_embed.shape[1] - 1
        if n_patch == n_pos and w == h:
            return self.pos_embed
        w0, h0, m = w // 14, h // 14, int(math.sqrt(n_pos))
        sx, sy = float(w0 + self.interpolate_offset) / m, float(h0 + self.interpolate_offset) / m
        grid = F.interpolate(self.pos_embed[:, 1:].reshape(1, m, m, -1).permute(0, 3, 1, 2), mode="bicubic", antialias=False, scale_factor=(sx, sy))
        assert (w0, h0) == tuple(grid.shape[-2:])
        return torch.cat([self.pos_embed[:, :1], grid.permute(0, 2, 3, 1).reshape(1, w0 * h0, -1)], 1)

    def forward(self, x):
        _, _, w, h = x.shape
        x = self.patch_embed(x)
        x = torch.cat([self.cls_token.expand(x.shape[0], -1, -1), x], 1)
        x = x + self.interpolate_pos_encoding(x, w, h)
        for blk in self.blocks:
            x = blk(x)
        return self.norm(x)[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    a = ap.parse_args()
    out, k64, s64, kp, sp = {}, {}, {}, {}, {}
    for case, c in v2.CASES.items():
        sd, image, x, b = v2.case_inputs(case)
        k64[case] = v2.image_keys(sd, x, -1, 1, image=image)
        s64[case] = v2.score(k64[case][:b], k64[case][b:])
        assert s64[case].min() > 1e-3, (case, s64[case])
        out[f"keys_{case}"], out[f"stride_{case}"], out[f"score_{case}"] = k64[case][:, ::c["stride"]].numpy(), np.int32(c["stride"]), s64[case].numpy()
        print(f"{case}: keys {tuple(k64[case].shape)} |K| max {k64[case].abs().max():.3f} scores {[round(v, 5) for v in s64[case].tolist()]}")
        for name, dt in DTYPES.items():
            k = v2.image_keys(sd, x, -1, 1, v2.Prec(dt), image=image)
            kp[case, name], sp[case, name] = (k - k64[case]).abs().max().item(), ((v2.score(k[:b], k[b:]) - s64[case]).abs() / s64[case]).max().item()
    for name in DTYPES:
        for case in v2.CASES:
            out[f"y_K_{case}_{name}"] = np.float64(kp[case, name])
        ya = max(sp["a20", name], sp["a64", name])
        for case, y in (("a20", ya), ("a64", ya), ("b", sp["b", name]), ("syn", sp["syn", name])):
            out[f"y_S_{case}_{name}"] = np.float64(y)
            print(f"y {case} {name}: keys {kp[case, name]:.3e} score {y:.3e}")

    e = v2.E2E
    sd_e = v2.random_state_dict(e["width"], e["layers"], e["table"], e["seed"])
    ref = load_reference(Path(a.reference), StandInDinov2(sd_e))
    src, edit = v2.make_images(1, e["s"], -1, 1, e["image_seed"])
    metric = ref.DinoVitStructure(input_range=(-1, 1), device="cpu", vit_model="dinov2_vits14")
    with torch.no_grad():
        e2e = float(metric.forward(edit.double(), src.double()))
        rk = metric.extractor.get_keys_from_input(metric.global_transform(((src[0].double() + 1) / 2))[None], layer_num=11)      # [heads][n][64]
        ke = v2.image_keys(sd_e, torch.cat([src, edit]), -1, 1)
    rk = rk.transpose(0, 1).reshape(rk.shape[1], -1)
    ours = float(v2.score(ke[:1], ke[1:])[0])
    print(f"reference class end to end: {e2e:.12g}, dinov2_ref {ours:.12g}, |diff| {abs(e2e - ours):.3e}; keys max |diff| {(rk - ke[0]).abs().max():.3e}")
    assert rk.shape == (257, 384) and (rk - ke[0]).abs().max() < 1e-9 and abs(e2e - ours) < 1e-10 * max(e2e, 1e-3) and repr(metric) == "dinov2_vits14"
    out["ref_e2e"], out["ref_keys"] = np.float64(e2e), rk[::16].numpy()
    path = ROOT / "tests" / "golden" / "dinov2_ref.npz"
    np.savez_compressed(path, **out)
    print(f"{path}: {path.stat().st_size / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
