#!/usr/bin/env python3
"""Metrics of a finished eval.py sweep (reference compute_metrics.py:20-126).

    python compute_metrics.py --data_path data/eval/PIE-Bench_v1 --output result/pie_etainv_ptp [--metric mse psnr ssim msssim]
                              [--batch 32] [--device cuda|cpu] [--size 512] [--limit N] [--categories 1_change_object ...]
                              [--clip_weights PATH|synthetic] [--clip_tokenizer DIR] [--clip_templates FILE] [--clip_model ViT-B/16]
                              [--dino_weights PATH|synthetic] [--dino_model dino_vitb8]
                              [--dinov2_weights PATH|synthetic] [--dinov2_model dinov2_vitb14]
                              [--lpips_weights PATH[,PATH]|synthetic] [--lpips_net alex]

Reads the layout eval.py writes, `<output>/imgs/{i:04d}_{source}_{target}.png`, next to the data set's source images.  Kept from the reference:
one `<output>/metrics/<name>.yaml` per metric, {name, mean, results: [{value, file}]}; a metric whose yaml exists is skipped (the file is
created exclusively before any work, so two runs never compute the same metric); a sample whose source or edited file is missing is skipped
with a message; a sample whose metric raises gets nan; both images go through StablePreprocess(size, center_crop=True).  Different by design:
samples are processed --batch at a time, all wanted metrics of a batch in one `image_metrics` call, and the default metric list is the four
that are built (EditMetric refuses the others by name).  The CLIP metrics (clip_text_img, clip_img_img, clip_textdir_imgdir, clip_text_img_acc) are
computed only when --clip_weights hands their weights over (a transformers CLIPModel state dict or an OpenAI clip checkpoint; "synthetic" with
--clip_model for dry runs): the data set's prompts go with every pair into one `clip_scores` call per batch.  --clip_templates FILE: one caption
template per line, each with a {} for the prompt.  dinovitstruct is computed only when --dino_weights hands DINO's checkpoint over ("synthetic" with
--dino_model for dry runs): one `dino_structure` call per batch; dinovitstruct_v2 likewise with --dinov2_weights (a published dinov2_vit{s,b,l}14
backbone checkpoint; "synthetic" with --dinov2_model).  lpips and bglpips are computed only when --lpips_weights hands the LPIPS AlexNet
over (one file in lpips.LPIPS's state-dict form, or backbone,heads; "synthetic" for dry runs): one `lpips_distance` call per batch and per name,
bglpips with the data set's foreground masks, which are 512 x 512: any other --size is refused for it."""
import argparse
import sys
from pathlib import Path

import torch
import yaml

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from dataset.pie_bench_data import PieBenchData, edit_image_name  # noqa: E402
from metrics import NAMES as IMAGE_NAMES  # noqa: E402
from metrics import EditMetric, image_metrics  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="image metrics of the PNGs an eval.py sweep wrote")
    ap.add_argument("--data_path", required=True)
    ap.add_argument("--output", required=True, help="the sweep's --output directory (holds imgs/; metrics/ is written next to it)")
    ap.add_argument("--metric", nargs="+", default=None, choices=EditMetric.get_available_metrics(), metavar="",
                    help="metric(s) to compute; default: the built ones (%s)" % " ".join(EditMetric.get_built_metrics()))
    ap.add_argument("--batch", type=int, default=32, help="image pairs per image_metrics call")
    ap.add_argument("--device", default=None, choices=["cuda", "cpu"], help="default: cuda when there is one")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--categories", nargs="+", default=None)
    ap.add_argument("--clip_weights", default=None, help="CLIP weights (a CLIPModel state dict, an OpenAI clip checkpoint, or 'synthetic'); "
                    "without it the clip_* metrics are refused")
    ap.add_argument("--clip_templates", default=None, help="file with one caption template per line, each with a {} for the prompt")
    ap.add_argument("--clip_model", default="ViT-B/16", help="geometry of --clip_weights synthetic")
    ap.add_argument("--clip_tokenizer", default=None, help="directory with CLIP's vocab.json and merges.txt (default: ETAINV_SD_PATH/tokenizer); "
                    "trained weights are refused without one")
    ap.add_argument("--dino_weights", default=None, help="DINO ViT weights (the published checkpoint, a state dict file, or 'synthetic'); without it "
                    "dinovitstruct is refused")
    ap.add_argument("--dino_model", default="dino_vitb8", help="the metric's model name; geometry of --dino_weights synthetic")
    ap.add_argument("--dinov2_weights", default=None, help="DINOv2 ViT weights (a published dinov2_vit{s,b,l}14 backbone checkpoint, a state dict file, "
                    "or 'synthetic'); without it dinovitstruct_v2 is refused")
    ap.add_argument("--dinov2_model", default="dinov2_vitb14", help="the metric's model name; geometry of --dinov2_weights synthetic")
    ap.add_argument("--lpips_weights", default=None, help="LPIPS AlexNet weights (lpips.LPIPS(net='alex').state_dict() form, or BACKBONE,HEADS: "
                    "torchvision's AlexNet and the lin layers; or 'synthetic'); without it lpips and bglpips are refused")
    ap.add_argument("--lpips_net", default="alex", help="widths of --lpips_weights synthetic: alex, or tiny for quick CPU runs")
    return ap.parse_args(argv)


def _claim(metric_dir: Path, metrics):
    """the metrics whose yaml this run creates (exclusive create, reference :44-51), with their files"""
    mine = []
    for m in metrics:
        f = metric_dir / f"{m.metric_name}.yaml"               # (the metric's name, not its repr: dinovitstruct prints its model's name)
        try:
            open(f, "x").close()
        except FileExistsError:
            print(f"skipping {f}")
            continue
        mine.append((m, f))
    return mine


_LPIPS = ("lpips", "bglpips")


def _compute(names, edits, sources, prompts, clip, dino=None, lpips=None, masks=None, dinov2=None):
    """{name: tensor [B]} of one batch: the image metrics in one `image_metrics` call, the CLIP metrics in one `clip_scores` call, dinovitstruct
    (and dinovitstruct_v2) in one `dino_structure` call, lpips and bglpips in one `lpips_distance` call each"""
    out = {}
    image = [n for n in names if n in IMAGE_NAMES]
    if image:
        out.update(image_metrics(torch.cat(edits), torch.cat(sources), (-1, 1), image))
    if "dinovitstruct" in names:
        from metrics import dino_structure
        out["dinovitstruct"] = dino_structure(torch.cat(edits), torch.cat(sources), dino, (-1, 1))
    if "dinovitstruct_v2" in names:
        from metrics import dino_structure
        out["dinovitstruct_v2"] = dino_structure(torch.cat(edits), torch.cat(sources), dinov2, (-1, 1))
    for n in names:
        if n in _LPIPS:
            from metrics import lpips_distance
            out[n] = lpips_distance(torch.cat(edits), torch.cat(sources), lpips, (-1, 1), mask=torch.stack(masks) if n == "bglpips" else None)
    other = [n for n in names if n not in IMAGE_NAMES and n not in ("dinovitstruct", "dinovitstruct_v2") and n not in _LPIPS]
    if other:
        from metrics import clip_scores
        out.update(clip_scores(torch.cat(edits), torch.cat(sources), [p[0] for p in prompts], [p[1] for p in prompts], other, clip, (-1, 1)))
    return out


def _values(names, edits, sources, prompts=None, clip=None, dino=None, lpips=None, masks=None, dinov2=None):
    """{name: [float per pair]}: one call for the batch; if it raises, pair by pair and metric by metric, nan where that raises"""
    prompts = prompts or [("", "")] * len(edits)
    masks = masks or [None] * len(edits)
    try:
        out = _compute(names, edits, sources, prompts, clip, dino, lpips, masks, dinov2)
        return {n: [float(v) for v in out[n].cpu()] for n in names}
    except Exception:
        pass
    vals = {n: [] for n in names}
    for e, s, p, k in zip(edits, sources, prompts, masks):
        for n in names:
            try:
                vals[n].append(float(_compute((n,), [e], [s], [p], clip, dino, lpips, [k], dinov2)[n][0]))
            except Exception as exc:
                print(f"{n}: nan because of {exc}")
                vals[n].append(float("nan"))
    return vals


@torch.no_grad()
def main(argv=None):
    a = parse_args(argv)
    device = a.device or ("cuda" if torch.cuda.is_available() else "cpu")
    clip = None
    if a.clip_weights is not None and any(m.startswith("clip_") for m in (a.metric or [])):
        from metrics import ClipModel
        templates = None
        if a.clip_templates is not None:
            with open(a.clip_templates) as fh:
                templates = [line.rstrip("\n") for line in fh if line.strip()]
        clip = ClipModel(a.clip_weights, device, a.clip_model, templates=templates, tokenizer=a.clip_tokenizer)
        if any(m != "clip_img_img" for m in a.metric if m.startswith("clip_")):
            clip.tokenize(["a"])                                 # trained weights without a CLIP tokenizer: refused here, before any yaml is claimed
    dino = None
    if a.dino_weights is not None and "dinovitstruct" in (a.metric or []):
        from metrics import DinoModel
        dino = DinoModel(a.dino_weights, device, a.dino_model)
    dinov2 = None
    if a.dinov2_weights is not None and "dinovitstruct_v2" in (a.metric or []):
        from metrics import Dinov2Model
        dinov2 = Dinov2Model(a.dinov2_weights, device, a.dinov2_model)
    lpips = None
    if a.lpips_weights is not None and any(m in _LPIPS for m in (a.metric or [])):
        if "bglpips" in a.metric and a.size != 512:            # refused here, before any yaml is claimed
            raise ValueError(f"bglpips takes the data set's 512 x 512 foreground masks: --size {a.size} is refused (the reference does not resize them either)")
        from metrics import LpipsModel
        paths = a.lpips_weights.split(",")
        lpips = LpipsModel(paths[0] if len(paths) == 1 else tuple(paths), device, a.lpips_net)
    own = lambda m: ({"clip_weights": clip} if clip is not None and m.startswith("clip_") else
                     {"dino_weights": dino, "dino_model": a.dino_model} if dino is not None and m == "dinovitstruct" else
                     {"dinov2_weights": dinov2, "dinov2_model": a.dinov2_model} if dinov2 is not None and m == "dinovitstruct_v2" else
                     {"lpips_weights": lpips, "lpips_net": a.lpips_net} if lpips is not None and m in _LPIPS else {})
    metrics = [EditMetric(m, input_range=(-1, 1), device=device, **own(m)) for m in (a.metric or EditMetric.get_built_metrics())]
    metric_dir = Path(a.output) / "metrics"
    metric_dir.mkdir(parents=True, exist_ok=True)
    mine = _claim(metric_dir, metrics)
    if not mine:
        return
    names = [m.metric_name for m, _ in mine]
    from modules.models import StablePreprocess
    preproc = StablePreprocess(device, size=a.size, center_crop=True)
    data = PieBenchData(a.data_path, skip_img_load=True, limit=a.limit, categories=a.categories)
    results = {n: [] for n in names}

    def flush(stems, edits, sources, prompts, masks):
        if not stems:
            return
        vals = _values(names, edits, sources, prompts, clip, dino, lpips, masks, dinov2)
        for (m, _), n in zip(mine, names):
            m.metric.losses.extend(vals[n])                      # what EditMetric.update records, for the whole batch
            results[n].extend({"value": v, "file": stem} for v, stem in zip(vals[n], stems))

    stems, edits, sources, prompts, masks = [], [], [], [], []
    for i in range(len(data)):
        s = data[i]
        edit_file = Path(a.output) / "imgs" / f"{edit_image_name(i, s['source_prompt'], s['edit']['target_prompt'])}.png"
        if not Path(s["image_file"]).exists() or not edit_file.exists():
            print(f"Skipping {edit_file}")
            continue
        try:
            e, src = preproc(edit_file), preproc(s["image_file"])
        except Exception as exc:                                 # an unreadable file: the sample's metrics "raise" (reference :97-107)
            print(f"Skipping {s['image_file']} because of {exc}")
            flush(stems, edits, sources, prompts, masks)         # (keeps the results in data-set order)
            stems, edits, sources, prompts, masks = [], [], [], [], []
            for (m, _), n in zip(mine, names):
                m.metric.losses.append(float("nan"))
                results[n].append({"value": float("nan"), "file": edit_file.stem})
            continue
        stems.append(edit_file.stem)
        edits.append(e)
        sources.append(src)
        prompts.append((s["source_prompt"], s["edit"]["target_prompt"]))
        masks.append(s["mask"])
        if len(stems) == a.batch:
            flush(stems, edits, sources, prompts, masks)
            stems, edits, sources, prompts, masks = [], [], [], [], []
    flush(stems, edits, sources, prompts, masks)
    for (m, f), n in zip(mine, names):
        res = {"name": n, "mean": m.compute()[0] if results[n] else float("nan"), "results": results[n]}
        with open(f, "w") as fh:
            yaml.dump(res, fh, Dumper=getattr(yaml, "CSafeDumper", yaml.SafeDumper))
        print(f"{n}: mean {res['mean']} over {len(results[n])} samples -> {f}")


if __name__ == "__main__":
    main()
