"""CPU checks of tests/cross_attention_ref.py: the restatement of the prompt-to-prompt cross edit against the oracle's controller (pinned to the reference by
tests/golden/ptp_algebra.npz), the table conventions, the coded inputs through the reference itself, and the condition that makes the GPU tests' bounds
legitimate: emulate_cross -- what any kernel of this kind must lose -- uses at most half of every bound on exactly the inputs those tests run."""
import json
import pathlib

import numpy as np
import pytest
import torch

from tests import cross_attention_ref as XR

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
HEADS = XR.HEADS


def _real_tables(n_img, replace):
    """tables of real prompt pairs (tests/golden/prompt_pairs.json): Refine + Reweight, or Replace + Reweight on the pair with equal word counts; a time blend with both values"""
    from oracle import ptp as optp
    pairs = json.loads((pathlib.Path(__file__).parent / "golden" / "prompt_pairs.json").read_text())
    tok = optp.WordTokenizer()
    tab = dict(mapper=[], alphas=[], equalizer=[], cross_alpha=[], replace_mat=[])
    for i in range(n_img):
        src, tgt = pairs[0] if replace else pairs[1 + i % 3]
        if replace:
            tab["replace_mat"].append(optp.replacement_mapper(src, tgt, tok))
        else:
            m, a = optp.refinement_mapper(src, tgt, tok)
            tab["mapper"].append(m)
            tab["alphas"].append(a)
        tab["equalizer"].append(optp.equalizer(tgt, (tgt.split(" ")[1 + i],), (2.0 + i,), tok))
        tab["cross_alpha"].append(optp.time_words_alpha([src, tgt], 10, {"default_": 0.4, tgt.split(" ")[1]: 0.9}, tok)[5, 0])
    T = lambda x, dt: torch.tensor(np.stack(x), dtype=dt) if x else None
    return {k: T(v, torch.int32 if k == "mapper" else torch.float32) for k, v in tab.items()}


@pytest.mark.parametrize("replace", [False, True])
def test_restatement_equals_the_oracle_controller(replace):
    from oracle import ptp as optp
    n_img, n, d = 2, 48, 40
    b = 4 * n_img
    q, kv = XR.random_q_kv(b, n, HEADS, d, XR.CTX, torch.float32, 1)
    tab = _real_tables(n_img, replace)
    assert 0 < float(tab["cross_alpha"].min()) + 1 and len(tab["cross_alpha"].unique()) >= 2        # the time blend keeps some words and not others
    out, probs = XR.ref_cross_attention(q, kv, HEADS, XR.CTX, 2, n_img, 0, tab)
    _, plain = XR.ref_cross_attention(q, kv, HEADS, XR.CTX, 0, n_img, 0, None)
    want = plain.clone()
    for img in range(n_img):
        rows = [img, n_img + img, 2 * n_img + img, 3 * n_img + img]
        ca = tab["cross_alpha"][img].numpy()[None, None].repeat(11, 0)
        kw = dict(replace_matrix=tab["replace_mat"][img].numpy()) if replace else dict(mapper=tab["mapper"][img].numpy().astype(np.int64), alphas=tab["alphas"][img].numpy())
        ctl = optp.AttentionEdit(10, ca, 0.6, equalizer=tab["equalizer"][img].numpy(), num_att_layers=1, **kw)
        want[rows] = ctl(plain[rows].reshape(4 * HEADS, n, XR.CTX).clone(), True, "up").reshape(4, HEADS, n, XR.CTX)
    assert float((want[3 * n_img:] - plain[3 * n_img:]).abs().max()) > 1e-3           # the edit did something ...
    assert torch.equal(want[:3 * n_img], plain[:3 * n_img])                            # ... to the cond-target rows only
    assert float((probs - want).abs().max()) < 1e-14
    k, v = kv.double().split(HEADS * d, dim=-1)
    ref_out = (want @ v.reshape(b, XR.CTX, HEADS, d).permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(b, n, HEADS * d)
    assert float((out - ref_out).abs().max()) < 1e-13
    # the three-row call is the last three row groups of the four-row call
    out3, probs3 = XR.ref_cross_attention(q[n_img:], kv[n_img:], HEADS, XR.CTX, 2, n_img, n_img, tab)
    assert torch.equal(out3, out[n_img:]) and torch.equal(probs3, probs[n_img:])


def test_table_conventions():
    g = torch.Generator().manual_seed(0)
    base, tg = torch.rand(5, 77, generator=g, dtype=torch.float64), torch.rand(5, 77, generator=g, dtype=torch.float64)
    ones = torch.ones(1, 77)
    mp = torch.randperm(77, generator=g).to(torch.int32)[None]
    a = torch.rand(1, 77, generator=g)
    # n_ctx = 77, no negative entry: python indexing
    got = XR.edit_probs(base, tg, dict(mapper=mp, alphas=a, cross_alpha=ones), 0, 77)
    assert torch.equal(got, base[:, mp[0].long()] * a[0].double() + tg * (1 - a[0].double()))
    # mapper -1 == 76 (and == n_ctx - 1 in a shorter context)
    m1, m76 = mp.clone(), mp.clone()
    m1[0, 3], m76[0, 3] = -1, 76
    assert torch.equal(XR.edit_probs(base, tg, dict(mapper=m1, alphas=ones, cross_alpha=ones), 0, 77), XR.edit_probs(base, tg, dict(mapper=m76, alphas=ones, cross_alpha=ones), 0, 77))
    short = torch.full((1, 77), -1, dtype=torch.int32)
    assert torch.equal(XR.edit_probs(base[:, :20], tg[:, :20], dict(mapper=short, alphas=ones, cross_alpha=ones), 0, 20), base[:, 19:20].expand(-1, 20))
    # absent tables: mapper 0, alpha 0, equalizer 1
    assert torch.equal(XR.edit_probs(base, tg, dict(alphas=ones, cross_alpha=ones), 0, 77), base[:, :1].expand(-1, 77))
    assert torch.equal(XR.edit_probs(base, tg, dict(mapper=mp, cross_alpha=ones), 0, 77), tg)
    # the equalizer multiplies BEFORE the time blend, and the blend keeps (1 - ca) of the target
    eq, ca = torch.full((1, 77), 3.0), torch.full((1, 77), 0.25)
    assert torch.allclose(XR.edit_probs(base, tg, dict(mapper=mp, alphas=ones, equalizer=eq, cross_alpha=ca), 0, 77), 0.75 * base[:, mp[0].long()] + 0.75 * tg, rtol=1e-15)
    # Replace: only the upper-left n_ctx x n_ctx block takes part
    mat = torch.rand(1, 77, 77, generator=g)
    poisoned = mat.clone()
    poisoned[0, 20:], poisoned[0, :, 20:] = float("nan"), float("nan")
    assert torch.equal(XR.edit_probs(base[:, :20], tg[:, :20], dict(replace_mat=poisoned, cross_alpha=ones), 0, 20), base[:, :20] @ mat[0, :20, :20].double())
    # mapper / replace_mat ask for the edit, which needs cross_alpha
    assert not XR.has_edit(None) and not XR.has_edit(dict(alphas=a, equalizer=eq, cross_alpha=ones)) and XR.has_edit(dict(replace_mat=mat, cross_alpha=ones))
    with pytest.raises(ValueError):
        XR.has_edit(dict(mapper=mp))


@pytest.mark.parametrize("n_ctx", [77, 20, 1])
def test_edit_tables_recipe(n_ctx):
    n_img = 3
    t, r = XR.edit_tables(n_img, n_ctx, 5), XR.edit_tables(n_img, n_ctx, 5, replace=True)
    assert r["mapper"] is None and r["alphas"] is None and t["replace_mat"] is None
    for img in range(n_img):
        mp, a, ca, eq = (t[k][img, :n_ctx] for k in ("mapper", "alphas", "cross_alpha", "equalizer"))
        neg = torch.nonzero(mp < 0).flatten()
        assert len(neg) == min(2, n_ctx) and (a[neg] != 0).all() and (ca[neg] != 0).all()
        assert sorted(mp[mp >= 0].tolist()) == sorted(set(mp[mp >= 0].tolist())) and int(mp.max()) < n_ctx
        idx = torch.arange(n_ctx)
        assert (a[(idx % 11 == 0) & (idx % 7 != 1)] == 1).all() and (a[1::7] == 0).all()           # (the zeros are written last: token 22 is 0)
        assert (ca[(idx % 13 == 0) & (idx % 9 != 2)] == 1).all() and (ca[2::9] == 0).all()
        assert float(eq.min()) >= 0.25 and float(eq.max()) <= 4 and float(r["replace_mat"][img, :n_ctx, :n_ctx].diagonal().min()) >= 0.5
        if n_ctx > 1:
            frac = lambda x: int(((x > 0) & (x < 1)).sum())
            assert frac(a) > n_ctx // 2 and frac(ca) > n_ctx // 2 and not torch.equal(t["alphas"][0, :n_ctx], t["alphas"][1, :n_ctx])
        if n_ctx < 77:
            assert t["alphas"][img, n_ctx:].isnan().all() and r["replace_mat"][img, n_ctx:].isnan().all() and r["replace_mat"][img, :, n_ctx:].isnan().all()


def test_ref_maps_slots():
    n_img, n, n_ctx = 2, 3, 20
    for layout, fr, rows, stored in [(1, 0, 2, {0: 0, 1: 0}), (1, 0, 4, {2: 0, 3: 0}), (2, 0, 8, {4: 0, 5: 0, 6: 1, 7: 1}), (2, 2, 6, {2: 0, 3: 0, 4: 1, 5: 1}),
                                     (3, 2, 6, {2: 1, 3: 1, 4: 0, 5: 0}), (3, 2, 4, {2: 1, 3: 1}), (0, 0, 4, {})]:
        probs = torch.arange(1, rows + 1, dtype=torch.float64)[:, None, None, None].expand(rows, HEADS, n, n_ctx).contiguous()
        maps = XR.ref_maps(probs, layout, n_img, fr, rows, 3, 1, 3, 2)
        assert maps.shape == (3, 3, 2, HEADS, n, 77)
        want = torch.zeros_like(maps)
        for r, slot in stored.items():
            want[1, r % n_img, slot, :, :, :n_ctx] = 2.0 * (r + 1)
        assert torch.equal(maps, want), (layout, fr, rows)
        assert torch.equal(XR.stored_mask(probs, layout, n_img, fr, rows, 3, 1, 3, 2), want != 0)


def _all_cases():
    for dtype in DTYPES:
        for c in XR.EDIT_CASES:
            yield "edit", dtype, c
        for c in XR.SHORT_CASES:
            yield "short", dtype, c
        for c in XR.STORE_CASES:
            yield "store", dtype, c


def _make(kind, dtype, c):
    if kind == "edit":
        return XR.edit_case(dtype, *c)
    if kind == "short":
        return XR.edit_case(dtype, *c[1:], n_ctx=c[0])
    return XR.store_case(dtype, *c)


def test_cases_cover_the_shapes():
    """every N, every d, both first rows, both edits and both gains at layout 2; both grids; both row counts of layouts 1 and 3"""
    e = XR.EDIT_CASES
    assert {c[0] for c in e} == {40, 200, 360} and {c[1] for c in e} == {40, 80, 160} and {c[2] for c in e} == {2, 4}
    assert {(c[0], c[1]) for c in e} >= {(n, d) for n in (200, 360) for d in (40, 80, 160)}
    assert {c[3] for c in e} == {0, 1} and {c[4] for c in e} == {"refine", "replace"} and {c[5] for c in e} == {1.0, 2.0}
    assert all(c[0] == 360 for c in e if c[2] == 4)
    assert {(c[0], c[2], c[5]) for c in XR.SHORT_CASES} == {(n_ctx, d, k) for n_ctx in (20, 1) for d in (40, 160) for k in ("refine", "replace")}
    assert {(c[0], c[1]) for c in XR.STORE_CASES} == {(1, 1), (1, 2), (3, 3), (3, 2)} and {c[2] for c in XR.STORE_CASES} == {200, 360}


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_uses_at_most_half_of_every_bound(dtype):
    """on exactly the inputs of tests/test_cross_attention_gpu.py (the same Case objects)"""
    worst = 0.0
    for kind, dt, c in _all_cases():
        if dt != dtype:
            continue
        case = _make(kind, dt, c)
        errs = XR.attn_errors(case.emu, case.ref, HEADS, case.d)[:3]
        ratios = [e / b for e, b in zip(errs, XR.bounds(dtype))]
        worst = max(worst, *ratios)
        assert max(ratios) <= 0.5, (case.label, errs, XR.bounds(dtype))
        # the map bound of the GPU tests: positive, and far below the global ceiling of 1e-3
        me = case.emulation_map_error()
        #   (one key: every probability is exactly 1 and the Refine edit of these tables exactly the equalizer -- the bound is 0 and the kernel must be exact)
        assert (0 < me or case.n_ctx == 1) and me * XR.MAP_MARGIN < 1e-4, (case.label, me)
    print(f"emulate_cross {dtype}: worst share of a bound {worst:.3f}")


@pytest.mark.parametrize("layout,fr,rows", [(0, 0, 8), (1, 0, 4), (1, 0, 8), (2, 0, 16), (2, 4, 12), (3, 4, 12), (3, 4, 8)])
def test_coded_roles_decode_through_the_reference(layout, fr, rows):
    n_img, n, d = 4, 5, 40
    q, kv = XR.coded_roles(rows, n, HEADS, d, torch.float16)
    tab = XR.identity_refine(n_img)
    out, probs = XR.ref_cross_attention(q, kv, HEADS, XR.CTX, layout, n_img, fr, tab)
    assert float(probs.amax(-1).min()) > 1 - 1e-10                     # >= 30 nats: the peak owns the softmax
    tok, row, slots = XR.expected_roles(layout, n_img, fr, rows, HEADS, edit=True)
    got_tok, got_row = XR.decode(out, HEADS, d)
    assert XR.first_mismatch(got_tok, tok[:, None, :], "token") is None
    assert XR.first_mismatch(got_row, row[:, None, None], "V row") is None
    if layout == 2:      # the premise: a c_t row names ANOTHER row's token, and all right pairs differ
        c_t = rows - n_img
        assert not torch.equal(tok[c_t], XR.role_token(c_t, c_t, torch.arange(HEADS))) and torch.equal(tok[c_t], tok[c_t - n_img])
    assert len({int(XR.role_token(r, r, 0)) for r in range(16)}) == 16
    if layout:
        maps = XR.ref_maps(probs, layout, n_img, fr, rows, 1, 0, n_img, 1)
        assert len(slots) == (2 * n_img if layout == 2 or rows == 3 * n_img else n_img)
        for (img, slot), want in slots.items():
            assert torch.equal(maps[0, img, slot].argmax(-1), want[:, None].expand(-1, n))
    # a wrong source row is seen: the four-row layout's c_t rows decoded as if unedited
    if layout == 2:
        wrong, _, _ = XR.expected_roles(layout, n_img, fr, rows, HEADS, edit=False)
        assert "row %d query 0 head 0" % (rows - n_img) in XR.first_mismatch(got_tok, wrong[:, None, :], "token")


@pytest.mark.parametrize("fr", [0, 1])
def test_coded_tables_decode_through_the_reference(fr):
    n_img, n, d = 4, 5, 40
    rows = (4 - fr) * n_img
    q, kv = XR.coded_tables_q_kv(rows, n, HEADS, d, torch.float16, 2)
    out, probs = XR.ref_cross_attention(q, kv, HEADS, XR.CTX, 2, n_img, fr * n_img, XR.coded_tables(n_img))
    got_tok, got_row = XR.decode(out, HEADS, d)
    c_t = rows - n_img
    want = XR.TABLE_TOKEN0 + torch.arange(n_img)
    assert XR.first_mismatch(got_tok[c_t:], want[:, None, None], "token") is None
    assert XR.first_mismatch(got_row, torch.arange(rows)[:, None, None], "V row") is None
    maps = XR.ref_maps(probs, 2, n_img, fr * n_img, rows, 1, 0, n_img, 1)
    for i in range(n_img):
        col = maps[0, i, 1, :, :, XR.TABLE_TOKEN0 + i]
        assert torch.equal(((col - 1) * 4).round().long(), torch.full_like(col, i, dtype=torch.long)) and float((col - (1 + i / 4)).abs().max()) < 1e-12
        rest = maps[0, i, 1].clone()
        rest[..., XR.TABLE_TOKEN0 + i] = 0
        assert float(rest.abs().max()) == 0.0


def test_attn_errors_finds_a_corrupted_row_head_query():
    case = XR.edit_case(torch.float16, *XR.EDIT_CASES[3])
    d = case.d
    out = case.ref.clone()
    out[5, 137, 6 * d:7 * d] *= 1.01
    g, blk, qry, where = XR.attn_errors(out, case.ref, HEADS, d)
    assert where["query"] == dict(row=5, head=6, query=137) and where["block"] == dict(row=5, head=6, block=137 // 32)
    assert abs(qry - 0.01) < 1e-9 and g < XR.TOL[torch.float16]          # invisible to the global measure, 2.5 times the single-query bound
    with pytest.raises(AssertionError):
        XR.check_attention(out, case.ref, HEADS, d, torch.float16)
