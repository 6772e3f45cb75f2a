"""Per-block UNet parity in plain torch, shared by tests/test_unet_blocks_ref.py (CPU) and tests/test_unet_blocks_gpu.py (test infrastructure).

A tap is the output of one block of the UNet graph, NHWC (rows, side * side, channels), named by the oracle module whose output it is
(oracle/unet.py): `time_embedding` (rows, 1, 4 ch0), `conv_in`, `down_blocks.{i}.resnets.{j}` / `.attentions.{j}` / `.downsamplers.0`, the three
blocks of `mid_block`, `up_blocks.{i}.resnets.{j}` / `.attentions.{j}` / `.upsamplers.0`, `conv_norm_out` (GroupNorm + SiLU, what conv_out reads).

  block_reference  one block of a float64 oracle on the TAPPED inputs of that block (teacher forcing): each block is judged on its own arithmetic
  block_stats      three distances of a tapped output to its reference: global, worst row / (row, channel) slice, worst element
  block_floor      the same three numbers for the emulated 16-bit execution of the block (oracle/lowprec.py; fp32: the fp32 oracle block)
  block_ratios     statistic / floor, per tap point: the quantity the tests bound by a margin"""
import math

import torch
import torch.nn.functional as F

from oracle import unet as ou
from oracle.lowprec import RoundingMode


def tap_names(unet):
    """the tap points of `unet` in execution order (the engine lists the same names: etainv_engine_tap_info)"""
    return list(block_inputs(unet))


def block_inputs(unet):
    """{tap name: (name of the tap the block reads, name of the skip tap concatenated to it or None)} in execution order, from the module tree"""
    g = {"time_embedding": (None, None), "conv_in": (None, None)}
    x, skips = "conv_in", ["conv_in"]
    for i, b in enumerate(unet.down_blocks):
        for j in range(len(b.resnets)):
            g[f"down_blocks.{i}.resnets.{j}"] = (x, None)
            x = f"down_blocks.{i}.resnets.{j}"
            if b.attentions is not None:
                g[f"down_blocks.{i}.attentions.{j}"] = (x, None)
                x = f"down_blocks.{i}.attentions.{j}"
            skips.append(x)
        if b.downsamplers is not None:
            g[f"down_blocks.{i}.downsamplers.0"] = (x, None)
            x = f"down_blocks.{i}.downsamplers.0"
            skips.append(x)
    for n in ("mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"):
        g[n] = (x, None)
        x = n
    for i, b in enumerate(unet.up_blocks):
        for j in range(len(b.resnets)):
            g[f"up_blocks.{i}.resnets.{j}"] = (x, skips.pop())
            x = f"up_blocks.{i}.resnets.{j}"
            if b.attentions is not None:
                g[f"up_blocks.{i}.attentions.{j}"] = (x, None)
                x = f"up_blocks.{i}.attentions.{j}"
        if b.upsamplers is not None:
            g[f"up_blocks.{i}.upsamplers.0"] = (x, None)
            x = f"up_blocks.{i}.upsamplers.0"
    g["conv_norm_out"] = (x, None)
    return g


def to_nhwc(y):
    return y.permute(0, 2, 3, 1).reshape(y.shape[0], -1, y.shape[1])


def to_nchw(x):
    side = math.isqrt(x.shape[1])
    assert side * side == x.shape[1]
    return x.reshape(x.shape[0], side, side, x.shape[2]).permute(0, 3, 1, 2)


def capture(unet, call):
    """{tap name: NHWC output} of every block during `call()` (one forward of `unet`, or of a wrapper around it), by forward hooks"""
    taps, hooks = {}, []

    def hook(name):
        def fn(mod, args, out):
            if name == "time_embedding":
                taps[name] = out[:, None, :]
            else:
                taps[name] = to_nhwc(F.silu(out) if name == "conv_norm_out" else out)
        return fn
    for n in tap_names(unet):
        hooks.append(unet.get_submodule(n).register_forward_hook(hook(n)))
    try:
        with torch.no_grad():
            call()
    finally:
        for h in hooks:
            h.remove()
    return taps


def timestep_embedding64(t, dim):
    """the sinusoidal embedding of oracle.unet.timestep_embedding with every step in float64: sin / cos of t * freq is conditioned by t (an fp32
    argument near 981 carries 6e-5 of rounding), so ANY fp32 evaluation of it is 1e-5 of the truth -- the fp32 floor of time_embedding includes it"""
    half = dim // 2
    args = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None, :]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def run_block(unet, name, taps, ctx, t, sample=None, rows=None, emb_dtype=None):
    """block `name` of `unet` on the tapped inputs of that block, in the dtype and on the device of `unet`'s parameters: NHWC output.
    t (rows,) int64 timesteps, sample (rows, 4, L, L) (conv_in only), `rows`: index list, the batch rows to run.  emb_dtype: the sinusoidal embedding is
    computed in fp32 (None: left so, as the oracle does) and rounded once to a 16-bit emb_dtype (what a 16-bit execution feeds time_embedding);
    torch.float64: computed in float64 throughout (timestep_embedding64)"""
    p = next(unet.parameters())

    def cv(x):
        x = x if rows is None else x[rows]
        return x.to(device=p.device, dtype=p.dtype)
    m = unet.get_submodule(name)
    prev, skip = block_inputs(unet)[name]
    with torch.no_grad():
        if name == "time_embedding":
            t = torch.as_tensor(t).reshape(-1)
            with torch._C.DisableTorchFunction():
                tt = t.cpu() if rows is None else t.cpu()[rows]
                emb = timestep_embedding64(tt, unet.ch0) if emb_dtype == torch.float64 else ou.timestep_embedding(tt, unet.ch0)
                if emb_dtype is not None:
                    emb = emb.to(emb_dtype)
                emb = emb.to(device=p.device, dtype=p.dtype)
            return m(emb)[:, None, :]
        if name == "conv_in":
            return to_nhwc(m(cv(sample)))
        x = to_nchw(cv(taps[prev]))
        if skip is not None:
            x = torch.cat([x, to_nchw(cv(taps[skip]))], dim=1)
        if ".resnets." in name:
            y = m(x, cv(taps["time_embedding"])[:, 0])
        elif ".attentions." in name:
            y = m(x, cv(ctx))
        elif name == "conv_norm_out":
            y = F.silu(m(x))
        else:
            y = m(x)
        return to_nhwc(y)


def _emb_dtype(dtype):
    return dtype if dtype in (torch.float16, torch.bfloat16) else torch.float64


def block_reference(unet64, name, taps, ctx, t, sample=None, rows=None, emb_dtype="auto"):
    """Teacher-forced float64 reference of one block: the submodule `name` of `unet64` (a .double() oracle) on the tapped input of the block --
    the tap of the preceding point, concatenated with the tapped skip for the up path's resnets, `time_embedding`'s tap as temb -- and the context
    and sample the caller rounded to the compute dtype.  NHWC float64.  emb_dtype: what the sinusoidal embedding is rounded to in front of
    time_embedding ("auto": the taps' dtype when it is a 16-bit one -- the engine keeps the embedding in the compute dtype; for fp32 taps the
    float64 sinusoid: the fp32 engine's own sinusoid is part of what is judged)"""
    if emb_dtype == "auto":
        emb_dtype = _emb_dtype(next(iter(taps.values())).dtype)
    return run_block(unet64, name, taps, ctx, t, sample, rows, emb_dtype=emb_dtype)


def block_stats(out, ref):
    """(a) rel L2 over the tensor; (b) the worst rel L2 over the (row) and the (row, channel) slices, a slice's denominator being its reference norm floored
    at the tensor RMS times sqrt(slice size) -- one wrong channel or row hides in (a); (c) the largest element error over the tensor RMS"""
    r = ref.double()
    d = out.to(r.device).double() - r
    assert d.dim() == 3 and d.shape == r.shape, (out.shape, ref.shape)
    rms = r.pow(2).mean().sqrt()

    def worst(dims):
        size = 1
        for k in dims:
            size *= r.shape[k]
        return (d.pow(2).sum(dims).sqrt() / r.pow(2).sum(dims).sqrt().clamp_min(rms * math.sqrt(size))).max()
    a = d.norm() / r.norm()
    b = torch.maximum(worst((1, 2)), worst((1,)))
    c = d.abs().max() / rms
    return float(a), float(b), float(c)


def block_floor(unet_lowprec, unet64, name, acts, ctx, t, sample, dtype, rows=None, emb_dtype="auto"):
    """block_stats of the reference-precision execution of one block against float64, both on `acts` (the inputs of the block) rounded to `dtype`:
    16-bit: `unet_lowprec` is an oracle.lowprec.LowPrecisionUNet of that dtype (parameters rounded once, every operator's output rounded under
    RoundingMode); fp32: `unet_lowprec` is the fp32 oracle itself"""
    prev, skip = block_inputs(unet64)[name]
    need = [n for n in (prev, skip) if n is not None] + (["time_embedding"] if ".resnets." in name else [])
    rd = {n: acts[n].to(dtype) for n in need}
    ctx_r, smp_r = ctx.to(dtype), (sample.to(dtype) if sample is not None else None)
    if emb_dtype == "auto":
        emb_dtype = _emb_dtype(dtype)
    ref = run_block(unet64, name, rd, ctx_r, t, smp_r, rows, emb_dtype=emb_dtype)
    if dtype == torch.float32:
        out = run_block(unet_lowprec, name, rd, ctx_r, t, smp_r, rows, emb_dtype=None if emb_dtype == torch.float64 else emb_dtype)
    else:
        assert unet_lowprec.lowdtype == dtype
        with RoundingMode(dtype):
            out = run_block(unet_lowprec.unet, name, rd, ctx_r, t, smp_r, rows, emb_dtype=emb_dtype)
    return block_stats(out, ref)


def block_ratios(stats, floors):
    """{name: (a, b, c) ratios statistic / floor}"""
    return {n: tuple(s / max(f, 1e-300) for s, f in zip(stats[n], floors[n])) for n in stats}


def flagged(ratios, margin, margins=None):
    """names whose worst ratio exceeds the margin (`margins`: documented per-tap exceptions to the common one)"""
    margins = margins or {}
    return [n for n, r in ratios.items() if max(r) > margins.get(n, margin)]


def format_table(title, names, cols, rows_of):
    """plain text table: one line per tap point, `rows_of(name)` -> the numbers under `cols`"""
    lines = [title, f"{'tap':<34}" + "".join(f"{c:>11}" for c in cols)]
    for n in names:
        lines.append(f"{n:<34}" + "".join(f"{v:>11.3g}" for v in rows_of(n)))
    return "\n".join(lines)
