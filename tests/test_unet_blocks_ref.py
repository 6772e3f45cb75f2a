"""The per-block check of tests/unet_blocks_ref.py catches what it is for (CPU, toy width).

The emulated reference-precision oracle (oracle/lowprec.py; the fp32 oracle for the fp32 case) stands in for the engine and forward hooks for its
taps.  Every block of the stand-in is compared with the float64 oracle block on the stand-in's own tapped inputs, and the three statistics are
divided by the floor of that block on the same inputs.  Without a defect the stand-in IS the floor's execution: every ratio is exactly 1.  With one
defect planted in one block, exactly that block exceeds the margin of the GPU test (2): no block before it (they never saw the defect) and none
after it (each is fed the tapped, already wrong, input and does its own arithmetic right) -- the localisation the whole-UNet tolerance lacks.

The GroupNorm eps defect (1e-6 for 1e-5) changes a block's output by about 4.5e-6 / variance: below the 16-bit floors, above the fp32 one, so it is
planted in the fp32 stand-in -- as on the GPU, where the fp32 engine's blocks are the ones that can see it."""
import copy

import pytest
import torch

from oracle.lowprec import LowPrecisionUNet
from oracle.unet import build_unet
from tests import unet_blocks_ref as ub

MARGIN = 2.0
TOY = dict(block_out_channels=(64, 128, 128, 128), groups=8, heads=4, cross_dim=32)
L, ROWS = 16, 3


@pytest.fixture(scope="module")
def toy():
    g = torch.Generator().manual_seed(3)
    return {"unet64": build_unet(0, **TOY).double(), "sample": torch.randn(ROWS, 4, L, L, generator=g), "ctx": torch.randn(ROWS, 77, 32, generator=g),
            "t": torch.tensor([0, 500, 981]), "fp32": build_unet(0, **TOY), torch.float16: LowPrecisionUNet(build_unet(0, **TOY), torch.float16),
            torch.bfloat16: LowPrecisionUNet(build_unet(0, **TOY), torch.bfloat16)}


def stand_in_taps(toy, dtype, plant=None):
    """taps of one free-running forward of the stand-in engine of `dtype`, with `plant(unet)` applied to a copy of it first"""
    net = copy.deepcopy(toy["fp32"] if dtype == torch.float32 else toy[dtype])
    unet = net if dtype == torch.float32 else net.unet
    if plant is not None:
        with torch.no_grad():
            plant(unet)
    smp, ctx = toy["sample"].to(dtype).float(), toy["ctx"].to(dtype).float()
    taps = ub.capture(unet, lambda: net(smp, toy["t"], encoder_hidden_states=ctx))
    return {n: v.to(dtype) for n, v in taps.items()}


def ratios_of(toy, dtype, taps):
    names = ub.tap_names(toy["unet64"])
    smp, ctx = toy["sample"].to(dtype), toy["ctx"].to(dtype)
    stats = {n: ub.block_stats(taps[n], ub.block_reference(toy["unet64"], n, taps, ctx, toy["t"], smp, emb_dtype=None)) for n in names}
    low = toy["fp32"] if dtype == torch.float32 else toy[dtype]
    floors = {n: ub.block_floor(low, toy["unet64"], n, taps, toy["ctx"], toy["t"], toy["sample"], dtype, emb_dtype=None) for n in names}   # (the
    # emulation feeds time_embedding the fp32 sinusoid, the engine a rounded one: emb_dtype)
    return stats, floors, ub.block_ratios(stats, floors)


def test_tap_names_and_graph():
    with torch.device("meta"):
        from oracle.unet import UNet2DConditionModel
        u = UNet2DConditionModel()
    g = ub.block_inputs(u)
    names = list(g)
    assert len(names) == 47 and names[:3] == ["time_embedding", "conv_in", "down_blocks.0.resnets.0"] and names[-1] == "conv_norm_out"
    assert g["up_blocks.0.resnets.0"] == ("mid_block.resnets.1", "down_blocks.3.resnets.1")
    assert g["up_blocks.0.resnets.2"] == ("up_blocks.0.resnets.1", "down_blocks.2.downsamplers.0")
    assert g["up_blocks.3.resnets.2"] == ("up_blocks.3.attentions.1", "conv_in")
    assert g["up_blocks.1.resnets.0"] == ("up_blocks.0.upsamplers.0", "down_blocks.2.attentions.1")
    assert "down_blocks.3.attentions.0" not in g and "up_blocks.3.upsamplers.0" not in g and "up_blocks.0.attentions.0" not in g


def test_block_stats_by_hand():
    ref = torch.ones(2, 4, 8, dtype=torch.float64)
    out = ref.clone()
    out[1, :, 3] += 0.5                                   # one (row, channel) slice off by 0.5: 4 of 64 elements
    a, b, c = ub.block_stats(out, ref)
    assert abs(a - 0.5 * 2 / 8) < 1e-12 and abs(b - 0.5) < 1e-12 and abs(c - 0.5) < 1e-12
    ref2 = ref.clone()
    ref2[1, :, 3] = 1e-3                                  # a slice far below the tensor RMS: its denominator is floored, not its own tiny norm
    out2 = ref2.clone()
    out2[1, :, 3] += 1e-3
    assert ub.block_stats(out2, ref2)[1] < 2e-3
    assert ub.block_stats(ref, ref) == (0.0, 0.0, 0.0)


def test_teacher_forced_blocks_compose_to_the_forward(toy):
    """the graph of block_inputs is the oracle's: in float64, every block run on the hooked input of that block reproduces the hooked output"""
    u = toy["unet64"]
    taps = ub.capture(u, lambda: u(toy["sample"].double(), toy["t"], encoder_hidden_states=toy["ctx"].double()))
    for n in ub.tap_names(u):
        ref = ub.block_reference(u, n, taps, toy["ctx"].double(), toy["t"], toy["sample"].double(), emb_dtype=None)
        assert ub.block_stats(taps[n], ref)[2] < 1e-12, n
    # the oracle's fp32 sinusoid against the float64 one: 1e-5-sized at t = 981, which is why the fp32 floor of time_embedding takes the float64 one
    exact = ub.block_reference(u, "time_embedding", taps, None, toy["t"])
    assert 1e-7 < ub.block_stats(taps["time_embedding"], exact)[2] < 1e-4
    part = ub.block_reference(u, "up_blocks.1.attentions.0", taps, toy["ctx"].double(), toy["t"], rows=[0, 2])
    assert torch.equal(part, ub.block_reference(u, "up_blocks.1.attentions.0", taps, toy["ctx"].double(), toy["t"])[[0, 2]])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_clean_stand_in_sits_on_the_floor(toy, dtype):
    stats, floors, ratios = ratios_of(toy, dtype, stand_in_taps(toy, dtype))
    for n, r in ratios.items():
        assert all(abs(v - 1.0) < 1e-9 for v in r), (n, r, stats[n], floors[n])
    assert all(min(f) > 0 for f in floors.values())


def _zero_bias(u):
    u.down_blocks[1].attentions[0].transformer_blocks[0].ff.net[2].bias.zero_()


def _gn_eps(u):
    u.mid_block.resnets[0].norm2.eps = 1e-6


def _time_row(u):
    u.up_blocks[1].resnets[1].time_emb_proj.register_forward_hook(lambda m, a, out: out.roll(1, 0))


def _softmax_scale(u):
    at = u.up_blocks[2].attentions[2].transformer_blocks[0].attn1
    at.scale = (2 * 128 // at.heads) ** -0.5


def _skip_swap(u):
    blk = u.up_blocks[0]
    inner = blk.forward

    def fwd(x, skips, temb, ctx):
        assert skips[-1].shape == skips[-2].shape
        skips[-1], skips[-2] = skips[-2], skips[-1]
        return inner(x, skips, temb, ctx)
    blk.forward = fwd


DEFECTS = {
    "linear_bias_zeroed": (_zero_bias, torch.float16, ["down_blocks.1.attentions.0"]),
    "groupnorm_eps": (_gn_eps, torch.float32, ["mid_block.resnets.0"]),
    "time_row_of_neighbour": (_time_row, torch.float16, ["up_blocks.1.resnets.1"]),
    "softmax_scale_wrong_head_dim": (_softmax_scale, torch.float16, ["up_blocks.2.attentions.2"]),
    # (a swap wrongs both blocks that read the two skips)
    "skip_swapped_with_neighbour": (_skip_swap, torch.float16, ["up_blocks.0.resnets.0", "up_blocks.0.resnets.1"]),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_flagged_in_its_block_only(toy, defect):
    plant, dtype, where = DEFECTS[defect]
    taps = stand_in_taps(toy, dtype, plant)
    clean = stand_in_taps(toy, dtype)
    names = ub.tap_names(toy["unet64"])
    first = names.index(where[0])
    assert all(torch.equal(taps[n], clean[n]) for n in names[:first]) and not torch.equal(taps[where[-1]], clean[where[-1]])
    assert not torch.equal(taps[names[-1]], clean[names[-1]])               # (the defect does reach the output: the later blocks pass on wrong inputs)
    _, _, ratios = ratios_of(toy, dtype, taps)
    print(defect, {n: tuple(round(v, 2) for v in ratios[n]) for n in where})
    assert ub.flagged(ratios, MARGIN) == where
    others = [max(ratios[n]) for n in names if n not in where]
    assert max(others) < 1.0 + 1e-9                                          # every other block is the floor's own execution of its tapped input


def test_one_channel_bias_hides_in_the_global_norm(toy):
    """one channel of one bias off by 3x the block's slice floor (statistic (b) of the floor, in units of the tensor RMS): the global rel L2 (a)
    stays inside the margin -- the channel is 1 / 64 of the energy -- and the slice statistic (b) flags the block"""
    dtype, name, ch = torch.float16, "down_blocks.0.attentions.1", 5
    clean = stand_in_taps(toy, dtype)
    _, floors, _ = ratios_of(toy, dtype, clean)
    rms = float(clean[name].double().pow(2).mean().sqrt())
    delta = 3.0 * floors[name][1] * rms

    def plant(u):
        u.down_blocks[0].attentions[1].proj_out.bias[ch] += delta
    taps = stand_in_taps(toy, dtype, plant)
    _, _, ratios = ratios_of(toy, dtype, taps)
    a, b, c = ratios[name]
    print(f"one-channel bias defect {delta:.2e}: ratios a {a:.2f} b {b:.2f} c {c:.2f}")
    assert a < MARGIN < b
    assert ub.flagged(ratios, MARGIN) == [name]
