"""Plain-PyTorch references for the cross-attention launches (no GPU needed, no import of the library): the 77-key softmax with the prompt-to-prompt edit
(Refine / Replace, Reweight, time blend) on the cond-target rows, the AttentionStore accumulation in every row layout, an emulation of what any such kernel
must lose, the edit-table recipe of the GPU tests, coded inputs whose outputs and stored maps name the rows / tokens / table entries they were computed from,
and the list of cases the GPU tests run.  tests/test_cross_attention_ref.py checks these helpers on the CPU; tests/test_cross_attention_gpu.py uses them.

Row layouts (roles per image: u_s / u_t = uncond source / target, c_s / c_t = cond source / target):
  0  no roles: nothing edited, nothing stored
  1  rows [u, c] x n_img or [c] x n_img (forward pass): cond rows stored in role slot 0
  2  rows [first_row, 4 n_img) of [u_s, u_t, c_s, c_t] x n_img, first_row 0 or n_img: c_t edited from c_s of the same image; c_s -> slot 0, c_t -> slot 1
  3  rows [u_t, c_t, c_s] x n_img, or [u_t, c_t] x n_img once the source rows have left: store only, c_t -> slot 1, c_s -> slot 0"""
import functools
import math

import torch

from tests.attention_ref import LOG2E, QUERY_FACTOR, TOL, attn_errors, bounds, check_attention  # noqa: F401  (re-exported: the GPU tests use them from here)

CTX = 77          # stride of every per-token table and of the map store
HEADS = 8


# ---------------------------------------------------------------------------------------------------------------- roles
def row_roles(layout, n_img, first_row, b):
    """[(role name or None, image)] of the b rows of a call"""
    if layout == 0:
        return [(None, 0)] * b
    if layout == 1:
        assert b in (n_img, 2 * n_img), (b, n_img)
        names = ["c"] if b == n_img else ["u", "c"]
    elif layout == 2:
        assert n_img >= 1 and first_row in (0, n_img) and b + first_row == 4 * n_img, (b, n_img, first_row)
        names = ["u_s", "u_t", "c_s", "c_t"][first_row // n_img:]
    else:
        assert layout == 3 and b in (2 * n_img, 3 * n_img), (layout, b, n_img)
        names = ["u_t", "c_t", "c_s"][: b // n_img]
    return [(name, img) for name in names for img in range(n_img)]


SLOT = {"c": 0, "c_s": 0, "c_t": 1}     # role slot of the map store; every other role is not stored


def source_rows(layout, n_img, first_row, b):
    """row -> the row whose probabilities the prompt-to-prompt edit injects into it (layout 2: c_t <- c_s of the same image), else -1"""
    roles = row_roles(layout, n_img, first_row, b)
    src = [-1] * b
    if layout == 2:
        for r, (name, img) in enumerate(roles):
            if name == "c_t":
                src[r] = roles.index(("c_s", img))
    return src


# ---------------------------------------------------------------------------------------------------------------- the edit
def has_edit(tables):
    """the rule of the library: mapper (Refine) or replace_mat (Replace) asks for the edit, and the edit needs the time blend's cross_alpha (the launcher refuses
    one without); alphas, equalizer or cross_alpha alone ask for nothing"""
    if not tables or (tables.get("mapper") is None and tables.get("replace_mat") is None):
        return False
    if tables.get("cross_alpha") is None:
        raise ValueError("edit without cross_alpha")
    return True


def edit_probs(base, tg, tab, img, n_ctx):
    """base, tg [..., n_ctx] (probabilities of the cond-source / cond-target row of image img) -> edited target probabilities, in the dtype of tg.
    rep = Replace ? base @ M : base[mapper] * a + tg * (1 - a);  rep *= eq;  p = rep * ca + (1 - ca) * tg.  Absent tables: mapper 0, alpha 0, equalizer 1;
    a negative mapper entry wraps by n_ctx; of replace_mat only the upper-left n_ctx x n_ctx block takes part."""
    dt = tg.dtype
    row = lambda name: None if tab.get(name) is None else tab[name][img, :n_ctx]
    if tab.get("replace_mat") is not None:
        rep = base @ tab["replace_mat"][img, :n_ctx, :n_ctx].to(dt)
    else:
        mp = row("mapper")
        mp = torch.zeros(n_ctx, dtype=torch.long) if mp is None else mp.long()
        mp = torch.where(mp < 0, mp + n_ctx, mp)
        assert int(mp.min()) >= 0 and int(mp.max()) < n_ctx, "mapper entry outside the context"
        a = row("alphas")
        a = torch.zeros(n_ctx, dtype=dt) if a is None else a.to(dt)
        rep = base[..., mp] * a + tg * (1 - a)
    if row("equalizer") is not None:
        rep = rep * row("equalizer").to(dt)
    ca = row("cross_alpha").to(dt)
    return rep * ca + (1 - ca) * tg


def _heads(t, heads):
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3)


def ref_cross_attention(q, kv, heads, n_ctx, layout, n_img, first_row, tables, dt=torch.float64):
    """q [b][N][C], kv [b][n_ctx][2C] -> (out [b][N][C], probabilities after the edit [b][heads][N][n_ctx]), `dt` arithmetic"""
    b, n, c = q.shape
    d = c // heads
    assert kv.shape == (b, n_ctx, 2 * c), (kv.shape, (b, n_ctx, 2 * c))
    k, v = kv.to(dt).split(c, dim=-1)
    probs = (_heads(q.to(dt), heads) @ _heads(k, heads).transpose(-1, -2) * d ** -0.5).softmax(-1)
    if has_edit(tables):
        plain = probs.clone()
        roles = row_roles(layout, n_img, first_row, b)
        for r, s in enumerate(source_rows(layout, n_img, first_row, b)):
            if s >= 0:
                probs[r] = edit_probs(plain[s], plain[r], tables, roles[r][1], n_ctx)
    out = (probs @ _heads(v, heads)).permute(0, 2, 1, 3).reshape(b, n, c)
    return out, probs


def emulate_cross(q, kv, heads, n_ctx, layout, n_img, first_row, tables, dtype):
    """What any kernel of this kind must lose: fp32 scores in log2 units, exp2, an fp32 sum and a reciprocal-multiply, the edit in fp32, P rounded to the
    operand type before P V (fp32 accumulation), the output rounded to the operand type.  Returns (out in dtype, its fp32 probabilities after the edit)."""
    b, n, c = q.shape
    d = c // heads
    f32 = torch.float32
    k, v = kv.to(f32).split(c, dim=-1)
    s = (_heads(q.to(f32), heads) @ _heads(k, heads).transpose(-1, -2)) * f32_scalar(d ** -0.5 * LOG2E)
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    probs = e * (1.0 / e.sum(-1, keepdim=True))
    if has_edit(tables):
        plain = probs.clone()
        roles = row_roles(layout, n_img, first_row, b)
        for r, src in enumerate(source_rows(layout, n_img, first_row, b)):
            if src >= 0:
                probs[r] = edit_probs(plain[src], plain[r], tables, roles[r][1], n_ctx)
    out = (probs.to(dtype).to(f32) @ _heads(v, heads)).permute(0, 2, 1, 3).reshape(b, n, c).to(dtype)
    return out, probs


def f32_scalar(x):
    return float(torch.tensor(x, dtype=torch.float32))


def ref_maps(probs, layout, n_img, first_row, rows, n_layers, map_layer, n_img_cap, calls):
    """The expected maps_acc [n_layers][n_img_cap][2][heads][N][77] after `calls` launches into layer map_layer of a zeroed store: cond rows only, in the
    role slot of the layout, columns >= n_ctx and every other entry exactly 0.  probs [rows][heads][N][n_ctx]."""
    _, heads, n, n_ctx = probs.shape
    assert probs.shape[0] == rows and n_img <= n_img_cap and 0 <= map_layer < n_layers
    maps = torch.zeros(n_layers, n_img_cap, 2, heads, n, CTX, dtype=probs.dtype)
    for r, (name, img) in enumerate(row_roles(layout, n_img, first_row, rows)):
        if name in SLOT:
            maps[map_layer, img, SLOT[name], :, :, :n_ctx] = probs[r] * calls
    return maps


def stored_mask(probs, *args):
    """True where ref_maps writes (the entries a launch may touch)"""
    return ref_maps(torch.ones_like(probs), *args) != 0


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_q_kv(b, n, heads, d, n_ctx, dtype, seed, gain=1.0):
    """standard normal, rounded to the operand type, Q and K multiplied by `gain` (the recipe of attention_ref.random_qkv)"""
    g = torch.Generator().manual_seed(seed)
    c = heads * d
    q = torch.randn(b, n, c, generator=g).to(dtype)
    kv = torch.randn(b, n_ctx, 2 * c, generator=g).to(dtype)
    if gain != 1.0:
        q *= gain
        kv[..., :c] *= gain
    return q, kv


def edit_tables(n_img, n_ctx, seed, replace=False):
    """Tables of stride 77 with a different draw per image, every term of the edit fractional somewhere and 0 / 1 somewhere:
      mapper       a random permutation of 0 .. n_ctx-1 with two entries -1 (at tokens whose alpha and cross_alpha are not 0, so that the wrap shows)
      alphas       U(0.1, 0.9), [::11] = 1, [1::7] = 0
      equalizer    U(0.25, 4)
      cross_alpha  U(0.1, 0.9), [::13] = 1, [2::9] = 0
      replace_mat  0.5 I + a 10 %-dense U(0, 1) matrix          (replace = True: given INSTEAD of mapper and alphas, as the library's callers do)
    Entries of tokens >= n_ctx are NaN (mapper: 0): nothing may read them.  (Tables that drive many keys to ca = a = 1 with unmapped source tokens shrink whole
    edited rows to ~1e-6, which fp16 P cannot hold: at n_ctx = 20, gain 3 the emulation alone exceeded the per-query bound 35 times.  Not this recipe.)"""
    mapper = torch.zeros(n_img, CTX, dtype=torch.int32)
    alphas, eq, ca = (torch.full((n_img, CTX), float("nan")) for _ in range(3))
    mat = torch.full((n_img, CTX, CTX), float("nan"))
    for img in range(n_img):
        g = torch.Generator().manual_seed(1000 * seed + img)
        u = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)
        a = u(0.1, 0.9, n_ctx)
        a[::11] = 1
        a[1::7] = 0
        c = u(0.1, 0.9, n_ctx)
        c[::13] = 1
        c[2::9] = 0
        mp = torch.randperm(n_ctx, generator=g).to(torch.int32)
        live = torch.nonzero((a != 0) & (c != 0)).flatten()
        mp[live[torch.randperm(len(live), generator=g)[:2]]] = -1
        alphas[img, :n_ctx], ca[img, :n_ctx], mapper[img, :n_ctx] = a, c, mp
        eq[img, :n_ctx] = u(0.25, 4.0, n_ctx)
        mat[img, :n_ctx, :n_ctx] = 0.5 * torch.eye(n_ctx) + (torch.rand(n_ctx, n_ctx, generator=g) < 0.1) * u(0.0, 1.0, n_ctx, n_ctx)
    if replace:
        return dict(mapper=None, alphas=None, equalizer=eq, cross_alpha=ca, replace_mat=mat)
    return dict(mapper=mapper, alphas=alphas, equalizer=eq, cross_alpha=ca, replace_mat=None)


def identity_refine(n_img):
    """mapper = arange, alphas = 1, cross_alpha = 1: the edited row takes the source row's probabilities as they are"""
    return dict(mapper=torch.arange(CTX, dtype=torch.int32).repeat(n_img, 1), alphas=torch.ones(n_img, CTX), equalizer=None,
                cross_alpha=torch.ones(n_img, CTX), replace_mat=None)


# ---------------------------------------------------------------------------------------------------------------- coded inputs
TOKEN_BITS, ROW_BITS, ROW_BIT0 = 7, 5, 8


def _coded_v(b, n_ctx, heads, d):
    """V of (row r, token j, every head): the token index in the signs of channels 0 .. 6, the row in the signs of channels 8 .. 12 (-1 / +1), 0 elsewhere.
    A non-negative combination of rows that agree in a bit keeps that sign, whatever the rounding."""
    assert n_ctx <= 1 << TOKEN_BITS and b <= 1 << ROW_BITS and d >= ROW_BIT0 + ROW_BITS
    v = torch.zeros(b, n_ctx, heads, d)
    v[..., :TOKEN_BITS] = (((torch.arange(n_ctx)[:, None] >> torch.arange(TOKEN_BITS)) & 1) * 2 - 1)[None, :, None].float()
    v[..., ROW_BIT0:ROW_BIT0 + ROW_BITS] = (((torch.arange(b)[:, None] >> torch.arange(ROW_BITS)) & 1) * 2 - 1)[:, None, None].float()
    return v


def decode(out, heads, d):
    """(token ids, row ids), each [b][N][heads], from the signs of an output"""
    o = out.float().reshape(out.shape[0], out.shape[1], heads, d)
    tok = ((o[..., :TOKEN_BITS] > 0).long() << torch.arange(TOKEN_BITS)).sum(-1)
    row = ((o[..., ROW_BIT0:ROW_BIT0 + ROW_BITS] > 0).long() << torch.arange(ROW_BITS)).sum(-1)
    return tok, row


def role_token(rq, rk, h):
    """the token that owns the softmax of (queries of row rq, keys of row rk, head h) of coded_roles"""
    return (rq + h - 3 * rk) % 32


def coded_roles(b, n, heads, d, dtype, n_ctx=CTX):
    """Q of (row rq, head h), every query, = s e_a with a = (rq + h) % 32; K of (row rk, head h), token j < 32, = s e_a' with a' = (j + 3 rk) % 32, tokens >= 32
    zero; s^2 d^-0.5 >= 30 nats.  The only non-zero score of (rq, rk, h) is at token role_token(rq, rk, h): for the right pair rq == rk == r that is
    (h - 2 r) % 32, different for every r < 16, and no pair with rq != rk gives the token of a right pair of the same rq (3 is invertible mod 32).
    V: _coded_v.  Returns (q, kv)."""
    assert d >= 32 and n_ctx >= 32 and b <= 16
    s = float(math.ceil(math.sqrt(31.5 * math.sqrt(d))))      # a small integer, exact in every operand type
    q = torch.zeros(b, n, heads, d)
    k = torch.zeros(b, n_ctx, heads, d)
    j = torch.arange(32)
    for r in range(b):
        for h in range(heads):
            q[r, :, h, (r + h) % 32] = s
            k[r, j, h, (j + 3 * r) % 32] = s
    kv = torch.cat([k.reshape(b, n_ctx, -1), _coded_v(b, n_ctx, heads, d).reshape(b, n_ctx, -1)], dim=-1)
    return q.reshape(b, n, -1).to(dtype), kv.to(dtype)


def expected_roles(layout, n_img, first_row, b, heads, edit):
    """(token [b][heads], row [b], map_token {(img, slot): [heads]}) that coded_roles must decode to: with the identity Refine a c_t row of layout 2 names
    (Q, K of its c_s row; V of itself) and its map slot names c_s; every other row and slot names itself."""
    src = source_rows(layout, n_img, first_row, b) if edit else [-1] * b
    h = torch.arange(heads)
    tok = torch.stack([role_token(s if s >= 0 else r, s if s >= 0 else r, h) for r, s in enumerate(src)])
    slots = {}
    for r, (name, img) in enumerate(row_roles(layout, n_img, first_row, b)):
        if name in SLOT:
            slots[img, SLOT[name]] = tok[r]
    return tok, torch.arange(b), slots


TABLE_TOKEN0 = 10


def coded_tables(n_img):
    """Replace tables: replace_mat of image i sends all mass to token 10 + i, equalizer_i[10 + i] = 1 + i / 4 (exact in fp32), cross_alpha = 1.  The edited
    row of image i is then equalizer_i[10 + i] * (sum of the source row = 1) at column 10 + i and 0 elsewhere, whatever Q and K are."""
    mat = torch.zeros(n_img, CTX, CTX)
    eq = torch.ones(n_img, CTX)
    for i in range(n_img):
        mat[i, :, TABLE_TOKEN0 + i] = 1
        eq[i, TABLE_TOKEN0 + i] = 1 + i / 4
    return dict(mapper=None, alphas=None, equalizer=eq, cross_alpha=torch.ones(n_img, CTX), replace_mat=mat)


def coded_tables_q_kv(b, n, heads, d, dtype, seed):
    """random Q and K, V of _coded_v"""
    q, kv = random_q_kv(b, n, heads, d, CTX, dtype, seed)
    kv[..., heads * d:] = _coded_v(b, CTX, heads, d).reshape(b, CTX, -1).to(dtype)
    return q, kv


def first_mismatch(got, want, what):
    """None, or a message naming the first (row, query, head) whose decoded id is wrong.  got, want broadcastable to [b][N][heads]."""
    want = want.expand_as(got)
    bad = torch.nonzero(got != want)
    if len(bad) == 0:
        return None
    r, qy, h = bad[0].tolist()
    return f"{what}: row {r} query {qy} head {h} decoded {int(got[r, qy, h])}, expected {int(want[r, qy, h])} ({len(bad)} wrong of {got.numel()})"


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' cases
# QT = 2: a block step of the 16-bit kernel is 128 queries.  N = 40: less than one wave's 32-query share, three waves wholly out of range; N = 200: one block per
# (row, head), two steps, the second ragged inside wave 2 and wave 3 clamped; N = 360: three query blocks on two blocks per (row, head): block 0 walks query blocks 0
# and 2 with the prefetch (d <= 80; d = 160 has none), the last is ragged.  n_img = 2: 3-D grids (first_row = 0); n_img = 4 at N = 360: the XCD-dealt 1-D grid in
# the plain and the edit launch (24 and 8 blocks per head at first_row = 0).
# (N, d, n_img, first_row in units of n_img, kind, gain)
EDIT_CASES = [
    (40, 40, 2, 0, "refine", 1.0),
    (40, 160, 2, 1, "replace", 2.0),
    (200, 40, 2, 1, "replace", 1.0),
    (200, 80, 2, 0, "refine", 2.0),
    (200, 160, 2, 0, "replace", 1.0),
    (360, 40, 2, 0, "refine", 2.0),
    (360, 80, 2, 1, "replace", 2.0),
    (360, 160, 2, 1, "refine", 1.0),
    (360, 40, 4, 0, "replace", 1.0),
    (360, 80, 4, 1, "refine", 2.0),
    (360, 160, 4, 0, "refine", 1.0),
    (40, 80, 2, 0, "replace", 1.0),
]
# (n_ctx, N, d, n_img, first_row in units of n_img, kind, gain)
SHORT_CASES = [(n_ctx, 200, d, 2, fr, kind, 1.0) for n_ctx in (20, 1) for d, fr in ((40, 0), (160, 1)) for kind in ("refine", "replace")]
# (layout, rows in units of n_img, N, d, n_img)
STORE_CASES = [(1, 1, 200, 40, 2), (1, 2, 360, 80, 2), (1, 2, 200, 160, 2), (3, 3, 200, 80, 2), (3, 2, 360, 40, 2), (3, 3, 360, 160, 4), (3, 2, 200, 160, 2)]
N_LAYERS, MAP_LAYER, CALLS = 3, 1, 2
MAP_MARGIN = 8.0


class Case:
    """one launch of the GPU tests with its float64 reference and its emulation, computed once per process"""

    def __init__(self, dtype, n, d, n_img, layout, rows, first_row, kind, gain, n_ctx=CTX, seed=0):
        self.dtype, self.n, self.d, self.n_img, self.layout, self.b, self.first_row, self.n_ctx = dtype, n, d, n_img, layout, rows, first_row, n_ctx
        self.q, self.kv = random_q_kv(rows, n, HEADS, d, n_ctx, dtype, 17 + seed, gain)
        self.tables = None if kind is None else edit_tables(n_img, n_ctx, 3 + seed, replace=kind == "replace")
        self.n_img_cap = n_img + 1
        edits = self.tables if layout == 2 else None        # layouts 1 and 3 store only, whatever tables the caller supplies
        args = (HEADS, n_ctx, layout, n_img, first_row, edits)
        self.ref, self.ref_probs = ref_cross_attention(self.q, self.kv, *args)
        self.emu, self.emu_probs = emulate_cross(self.q, self.kv, *args, dtype)
        self.label = f"N={n} d={d} n_img={n_img} layout={layout} rows={rows} first_row={first_row} n_ctx={n_ctx} {kind} gain={gain:g}"

    def map_args(self):
        return (self.layout, self.n_img, self.first_row, self.b, N_LAYERS, MAP_LAYER, self.n_img_cap, CALLS)

    def emulation_map_error(self):
        """worst absolute error of the emulation's fp32 probabilities against float64"""
        return float((self.emu_probs.double() - self.ref_probs).abs().max())


@functools.lru_cache(maxsize=None)
def edit_case(dtype, n, d, n_img, fr, kind, gain, n_ctx=CTX):
    return Case(dtype, n, d, n_img, 2, (4 - fr) * n_img, fr * n_img, kind, gain, n_ctx, seed=n + d)


@functools.lru_cache(maxsize=None)
def store_case(dtype, layout, rows, n, d, n_img):
    # (layout 3 is called with edit tables: it must ignore them)
    return Case(dtype, n, d, n_img, layout, rows * n_img, n_img if layout == 3 else 0, "refine" if layout == 3 else None, 1.0, seed=n + d + layout)


# ---------------------------------------------------------------------------------------------------------------- calls the launcher must refuse
# Overrides of REFUSAL_BASE (a valid prompt-to-prompt call: 4 n_img rows, Refine tables, store on) and a piece of the message each must leave in etainv_last_error.
# tests/test_host_logic.py runs them without a GPU (a refusal comes before any launch), tests/test_cross_attention_gpu.py with sentinel-filled tensors.
REFUSAL_BASE = dict(mode="ptp", n_img=2, b=8, first_row=0, src_exit_block=0, n_ctx=CTX, d=40, store=1, maps=True, n_img_cap=2, mapper=True, cross_alpha=True)
REFUSALS = [
    ("layout 2, n_img = 0", dict(n_img=0), "n_img >= 1"),
    ("layout 2, n_img = 2 with 4 rows (the first cond-target row would be row 6)", dict(b=4), "prompt-to-prompt layout"),
    ("layout 2, 3 n_img rows without first_row", dict(b=6), "prompt-to-prompt layout"),
    ("layout 2, first_row = n_img with 4 n_img rows", dict(first_row=2), "prompt-to-prompt layout"),
    ("layout 2, first_row = 1 with 4 n_img - 1 rows", dict(first_row=1, b=7), "prompt-to-prompt layout"),
    ("layout 2, first_row = 2 n_img with 2 n_img rows", dict(first_row=4, b=4), "prompt-to-prompt layout"),
    ("layout 3, 4 n_img rows", dict(src_exit_block=12, first_row=2, b=8, mapper=False), "[u_t, c_t, c_s]"),
    ("layout 3, n_img rows", dict(src_exit_block=12, first_row=2, b=2, mapper=False), "[u_t, c_t, c_s]"),
    ("layout 1, 3 n_img rows", dict(mode="store", b=6, mapper=False), "store layout"),
    ("layout 1, n_img + 1 rows", dict(mode="store", b=3, mapper=False), "store layout"),
    ("edit without cross_alpha", dict(cross_alpha=False), "without cross_alpha"),
    ("store without maps_acc", dict(maps=False), "maps_acc missing"),
    ("store with n_img > n_img_cap", dict(n_img_cap=1), "n_img > n_img_cap"),
    ("n_ctx = 0", dict(n_ctx=0), "n_ctx"),
    ("n_ctx = 78", dict(n_ctx=78), "n_ctx"),
    ("head_dim 64", dict(d=64), "head_dim"),
]
