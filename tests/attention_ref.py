"""Plain-PyTorch references for the self-attention launches (no GPU needed, no import of the library): the two QKV layouts, the engine's pre-scaled
queries, the batch-row couplings of the prompt-to-prompt / MasaCtrl modes in all three row layouts, per-item error measures, an emulation of what any
16-bit flash kernel must lose, and coded inputs whose outputs name the rows / tokens they were computed from.
tests/test_attention_ref.py checks these helpers on the CPU; the GPU tests (test_kernels_gpu.py, test_attention_forms_gpu.py) use them."""
import math

import torch

LOG2E = 1.4426950408889634
TOL = {torch.float16: 2e-3, torch.bfloat16: 1.2e-2, torch.float32: 2e-5}   # the per-kernel tolerances of tests/test_kernels_gpu.py (relative L2, fp32 accumulation)
QUERY_FACTOR = 2.0                                      # ... and its factor for a single query


# ---------------------------------------------------------------------------------------------------------------- layouts
def to_head_major(qkv, heads):
    """rows [b][n][3][heads][d] -> three planes [3][b][heads][n][d]"""
    b, n, c3 = qkv.shape
    d = c3 // (3 * heads)
    return qkv.reshape(b, n, 3, heads, d).permute(2, 0, 3, 1, 4).contiguous()


def from_head_major(planes, b, n, heads):
    d = planes.numel() // (3 * b * heads * n)
    return planes.reshape(3, b, heads, n, d).permute(1, 3, 0, 2, 4).reshape(b, n, 3 * heads * d).contiguous()


def prescale_q(qkv, heads, d):
    """What the engine's to_q projection emits when the softmax scale is folded into its weights: q' = round(q * d^-0.5 * log2 e)."""
    out = qkv.clone()
    c = heads * d
    out[..., :c] = (qkv[..., :c].float() * (d ** -0.5 * LOG2E)).to(qkv.dtype)
    return out


# ---------------------------------------------------------------------------------------------------------------- row couplings
def row_maps(b, n_img, mode, first_row):
    """(qmap, kmap, vmap): the batch rows of THIS call that output row r takes its queries, keys and values from.
    Roles per image: u_s / u_t = uncond source / target, c_s / c_t = cond source / target.
      first_row == 0      rows [u_s, u_t, c_s, c_t] x n_img
      first_row == n_img  rows [u_t, c_s, c_t] x n_img          (mode 1 only)
      first_row < 0       rows [u_t, c_t, c_s] x n_img          (mode 1 only)
    mode 1 (prompt-to-prompt self-replace): c_t attends with the Q and K of c_s of the same image;
    mode 2 (MasaCtrl): u_t takes K and V of u_s, c_t takes K and V of c_s."""
    ident = torch.arange(b)
    if mode == 0:
        return ident, ident.clone(), ident.clone()
    if first_row == 0:
        roles = ["u_s", "u_t", "c_s", "c_t"]
    elif first_row < 0:
        roles = ["u_t", "c_t", "c_s"]
    else:
        assert first_row == n_img
        roles = ["u_t", "c_s", "c_t"]
    assert b == len(roles) * n_img, (b, n_img, first_row)
    assert mode == 1 or len(roles) == 4, "MasaCtrl needs all four roles"
    row_of = {(role, img): i * n_img + img for i, role in enumerate(roles) for img in range(n_img)}
    qmap, kmap, vmap = ident.clone(), ident.clone(), ident.clone()
    for img in range(n_img):
        if mode == 1:
            qmap[row_of["c_t", img]] = kmap[row_of["c_t", img]] = row_of["c_s", img]
        else:
            for tgt, src in (("u_t", "u_s"), ("c_t", "c_s")):
                kmap[row_of[tgt, img]] = vmap[row_of[tgt, img]] = row_of[src, img]
    return qmap, kmap, vmap


def rows_in_four_row_call(n_img, first_row):
    """For a three-row call: the row of the four-row tensor [u_s, u_t, c_s, c_t] x n_img that each of its rows is."""
    order = [1, 3, 2] if first_row < 0 else [1, 2, 3]
    return torch.tensor([role * n_img + img for role in order for img in range(n_img)])


# ---------------------------------------------------------------------------------------------------------------- references
def _split(qkv, heads, maps, dt):
    b, n, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    q, k, v = qkv.split(c, dim=-1)
    if maps is not None:
        qm, km, vm = (m.to(qkv.device) for m in maps)
        q, k, v = q[qm], k[km], v[vm]
    sp = lambda t: t.to(dt).reshape(b, n, heads, d).permute(0, 2, 1, 3)
    return sp(q), sp(k), sp(v), d


def ref_self_attention(qkv, heads, qmap=None, kmap=None, vmap=None, prescaled=False, dt=torch.float32, max_bytes=2 << 30):
    """softmax(q k^T d^-0.5) v per (row, head) on the device of qkv, `dt` arithmetic.  prescaled: the queries are q' of prescale_q and the
    probabilities are softmax(ln 2 * q' k^T) of the ROUNDED q' (the rounding of the projection's output is not the attention kernel's error).
    Rows are processed in groups whose score tensor stays below max_bytes."""
    b, n, c3 = qkv.shape
    maps = None if qmap is None else (qmap, kmap, vmap)
    q, k, v, d = _split(qkv, heads, maps, dt)
    scale = math.log(2.0) if prescaled else d ** -0.5
    out = torch.empty(b, n, c3 // 3, dtype=dt, device=qkv.device)
    step = max(1, int(max_bytes // (heads * n * n * torch.finfo(dt).bits // 8)))
    for r0 in range(0, b, step):
        a = (q[r0:r0 + step] @ k[r0:r0 + step].transpose(-1, -2) * scale).softmax(-1)
        out[r0:r0 + step] = (a @ v[r0:r0 + step]).permute(0, 2, 1, 3).reshape(-1, n, c3 // 3)
    return out


def emulate_16bit(qkv, heads, qmap=None, kmap=None, vmap=None, prescaled=False, chunk=1024):
    """The error no 16-bit flash kernel can avoid: exact (float64) scores and row maximum, the probabilities P = exp(s - m) ROUNDED to the operand type,
    P V and the denominator sum(P) accumulated in fp32, the quotient rounded to the operand type."""
    b, n, c3 = qkv.shape
    dtype = qkv.dtype
    maps = None if qmap is None else (qmap, kmap, vmap)
    q, k, v, d = _split(qkv, heads, maps, torch.float64)
    scale = math.log(2.0) if prescaled else d ** -0.5
    v32 = v.float()
    out = torch.empty(b, heads, n, d, dtype=dtype, device=qkv.device)
    chunk = max(32, min(chunk, int((1 << 31) // (b * heads * n * 8))))   # scores of a query chunk: at most 2 GB
    for q0 in range(0, n, chunk):
        s = q[:, :, q0:q0 + chunk] @ k.transpose(-1, -2) * scale
        p = (s - s.amax(-1, keepdim=True)).exp().to(dtype).float()
        out[:, :, q0:q0 + chunk] = ((p @ v32) / p.sum(-1, keepdim=True)).to(dtype)
    return out.permute(0, 2, 1, 3).reshape(b, n, c3 // 3)


# ---------------------------------------------------------------------------------------------------------------- error measures
def attn_errors(out, ref, heads, d):
    """(global, worst 32-query block of a (row, head), worst single query of a (row, head)) relative L2 errors + where the two maxima are."""
    b, n, c = out.shape
    assert c == heads * d and ref.shape == out.shape
    e2 = (out.double() - ref.double()).reshape(b, n, heads, d).square().sum(-1)   # [b][n][heads]
    r2 = ref.double().reshape(b, n, heads, d).square().sum(-1)
    glob = (e2.sum() / r2.sum().clamp_min(1e-300)).sqrt().item()
    nb = (n + 31) // 32
    pad = nb * 32 - n
    blk = lambda t: torch.nn.functional.pad(t, (0, 0, 0, pad)).reshape(b, nb, 32, heads).sum(2)   # [b][nb][heads]
    rb = (blk(e2) / blk(r2).clamp_min(1e-300)).sqrt()
    rq = (e2 / r2.clamp_min(1e-300)).sqrt()
    ib, iq = int(rb.argmax()), int(rq.argmax())
    where = {"block": dict(row=ib // (nb * heads), head=ib % heads, block=ib // heads % nb),
             "query": dict(row=iq // (n * heads), head=iq % heads, query=iq // heads % n)}
    return glob, rb.max().item(), rq.max().item(), where


def bounds(dtype, factor=1.0):
    """(global, per 32-query block, per query) bounds: the file's tolerance at all three grains, the single-query factor on the last."""
    return TOL[dtype] * factor, TOL[dtype] * factor, QUERY_FACTOR * TOL[dtype] * factor


ROUTES = ["d40-one-block-per-wave", "d40-persistent", "d40-two-block", "d80-persistent", "d80", "d160"]   # in the order of enum SelfAttnRoute


def self_attention_route(b, n, heads, d, n_cu, persist40=True, persist80=True):
    """Which kernel a 16-bit launch takes; the tests assert their premises with it.  A mirror of self_attn_route (csrc/self_attn_route.h), the rule the launcher
    switches on: test_attention_ref.py compiles that header and compares the two.  persist40 / persist80: ETAINV_A40_PERSIST / ETAINV_A80_PERSIST (default on)."""
    def persistent(item_queries):
        return (n % item_queries == 0 and n % 256 == 0 and n >= 1024 and 3 * b * n * heads * d * 2 < 1 << 32
                and (n // item_queries) * heads * b >= 2 * n_cu)
    if d == 40:
        if -(-n // 256) * heads * b <= 256 and n > 128:
            return "d40-one-block-per-wave"
        return "d40-persistent" if persist40 and persistent(512) else "d40-two-block"
    if d == 80:
        return "d80-persistent" if persist80 and persistent(256) else "d80"
    return "d160"


def check_attention(out, ref, heads, d, dtype, factor=1.0, label="", emulate=None, query_ref=None):
    """Assert the three bounds; prints the measured values (pytest -s).  With ETAINV_ATTN_MARGINS=1 and `emulate` (a callable returning emulate_16bit of the
    same input) the emulation's three errors are printed beside them (profiles/attention_parity_margins.log is such a run).
    query_ref: the single-query error is measured against this reference instead (test_self_attention_d40_maximum_jumps_late says when and why)."""
    import os
    g, blk, qry, where = attn_errors(out, ref, heads, d)
    if query_ref is not None:
        _, _, qry, wq = attn_errors(out, query_ref, heads, d)
        where["query"] = wq["query"]
        label += " query-vs-rounded-q"
    bg, bb, bq = bounds(dtype, factor)
    line = (f"attention-parity {label} dtype={str(dtype).split('.')[-1]} shape={tuple(out.shape)} d={d} kernel: global={g:.3e} block={blk:.3e} query={qry:.3e} "
            f"bounds: {bg:.1e} {bb:.1e} {bq:.1e}")
    if emulate is not None and os.environ.get("ETAINV_ATTN_MARGINS") == "1":
        eg, eb, eq, _ = attn_errors(emulate(), ref, heads, d)
        line += f" emulation: global={eg:.3e} block={eb:.3e} query={eq:.3e} ok={int(g < bg and blk < bb and qry < bq and max(eg / bg, eb / bb, eq / bq) <= 0.5)}"
    print(line)
    assert math.isfinite(g) and g < bg, (label, "global", g, bg)
    assert blk < bb, (label, "32-query block", blk, bb, where["block"])
    assert qry < bq, (label, "query", qry, bq, where["query"])
    return g, blk, qry


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_qkv(b, n, heads, d, dtype, seed, gain=1.0):
    """The input recipe of the kernel tests: standard normal, rounded to the operand type, Q and K multiplied by `gain`."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(b, n, 3 * heads * d, generator=g).to(dtype)
    if gain != 1.0:
        qkv[..., : 2 * heads * d] *= gain
    return qkv


def _boost(qkv, heads, d, row, head, key, query, log2_gain):
    # score(query, key) of (row, head) ~ log2_gain * ln 2 above that query's typical maximum: k := q * t with t = gain / (|q|^2 * scale)
    c = heads * d
    qv = qkv[row, query, head * d:(head + 1) * d].float()
    t = (log2_gain * 0.6931 + 6.0) / (float(qv @ qv) * d ** -0.5)
    qkv[row, key, c + head * d: c + (head + 1) * d] = (qv * t).to(qkv.dtype)


SPECULATIVE_ITEMS = [(2, 3, 1500, 300)]                                         # (row, head, key, query) of test_self_attention_d40_speculative_maximum
EXACT_PASS_ITEMS = [(2, 3, 1500, 300), (7, 0, 100, 1999), (15, 7, 2047, 0)]      # ... of test_self_attention_d40_persistent_kernel_exact_pass


def speculative_maximum_qkv(b, heads, n, d, dtype, seed, overflow_items):
    """Four regimes of the deferred reference maximum, each in its own batch row: row 0 plain; row 1 late keys 2^6 .. 2^12 above the first tile's maximum for
    some queries; `overflow_items` (row, head, key, query): one late key ~2^40 above it (fp16 P overflows); row 3 the first tile far below everything else."""
    qkv = random_qkv(b, n, heads, d, dtype, seed)
    c = heads * d
    for i, (key, g) in enumerate([(700, 6), (1300, 9), (2000, 12), (1999, 8)]):
        _boost(qkv, heads, d, 1, i % heads, key, 64 * i + 7, g)
    for row, head, key, query in overflow_items:
        _boost(qkv, heads, d, row, head, key, query, 40)
    qkv[3, :64, c:2 * c] = (qkv[3, :64, c:2 * c] * 0.02).to(dtype)
    qkv[3, :, :c] = (qkv[3, :, :c] * 3).to(dtype)
    return qkv


def maximum_jumps_late_qkv(dtype=torch.float16):
    """b = 1, 8 heads, N = 512, d = 40: keys far above the running maximum in late tiles for queries 5 and 130, a strongly negative first tile for query 200."""
    heads, n, d = 8, 512, 40
    c = heads * d
    qkv = random_qkv(1, n, heads, d, dtype, 77)
    q, k = qkv[..., :c], qkv[..., c:2 * c]
    k[0, 300] = (q[0, 5] * 6).to(dtype)
    k[0, 450] = (q[0, 130] * 8).to(dtype)
    k[0, :64] = (k[0, :64] - 4 * q[0, 200:201]).to(dtype)
    return qkv


# ---------------------------------------------------------------------------------------------------------------- coded inputs
def coded_v_qkv(b, n, heads, d, dtype, seed):
    """Random Q, K; V of (row r, head h), every token, carries id = r * heads + h as signs: channel c < 8 is +1 if bit c of id is set, else -1.
    A convex combination of such rows keeps the signs, whatever the rounding."""
    assert b * heads <= 256 and d >= 8
    qkv = random_qkv(b, n, heads, d, dtype, seed)
    v = qkv[..., 2 * heads * d:].reshape(b, n, heads, d)
    ids = torch.arange(b)[:, None] * heads + torch.arange(heads)[None]                     # [b][heads]
    bits = ((ids[..., None] >> torch.arange(8)) & 1) * 2 - 1                               # [b][heads][8]
    v[..., :8] = bits[:, None].to(dtype)
    return qkv


def decode_v_ids(out, heads, d):
    """[b][n][heads] ids read from the signs of channels 0 .. 7"""
    o = out.float().reshape(out.shape[0], out.shape[1], heads, d)[..., :8]
    return ((o > 0).long() << torch.arange(8, device=out.device)).sum(-1)


TOKEN_BITS = 12


def coded_qk_qkv(b, n, heads, d, dtype):
    """Q of (row r, head h) = s e_a for every query, a = (r + h) % 32; K of (row r', head h) is zero except token 32 r' + a' = s e_a' (a' = 0 .. 31);
    V (every row and head) carries the token index in the signs of channels 0 .. 11.  The query of an output row that takes Q from row rq and K from
    row rk has its only non-zero score, s^2 d^-0.5 >= 30 nats, at token 32 rk + (rq + h) % 32: the peak owns the softmax and the output's signs name it."""
    assert d >= 32 and n >= 32 * b and n <= 1 << TOKEN_BITS
    s = float(math.ceil(math.sqrt(31.5 * math.sqrt(d))))   # a small integer (exact in both types) with s^2 d^-0.5 >= 31.5: 30 nats also after prescale_q rounds q'
    q = torch.zeros(b, n, heads, d)
    k = torch.zeros(b, n, heads, d)
    for r in range(b):
        for h in range(heads):
            q[r, :, h, (r + h) % 32] = s
            k[r, 32 * r + torch.arange(32), h, torch.arange(32)] = s
    v = torch.zeros(b, n, heads, d)
    bits = ((torch.arange(n)[:, None] >> torch.arange(TOKEN_BITS)) & 1) * 2 - 1
    v[..., :TOKEN_BITS] = bits[None, :, None].float()
    return torch.cat([q.reshape(b, n, -1), k.reshape(b, n, -1), v.reshape(b, n, -1)], dim=-1).to(dtype)


def decode_tokens(out, heads, d):
    o = out.float().reshape(out.shape[0], out.shape[1], heads, d)[..., :TOKEN_BITS]
    return ((o > 0).long() << torch.arange(TOKEN_BITS, device=out.device)).sum(-1)


def expected_tokens(qmap, kmap, n, heads):
    """[b][n][heads]"""
    h = torch.arange(heads)
    t = 32 * kmap[:, None] + (qmap[:, None] + h[None]) % 32
    return t[:, None, :].expand(-1, n, -1)


def expected_v_ids(vmap, n, heads):
    return (vmap[:, None] * heads + torch.arange(heads)[None])[:, None, :].expand(-1, n, -1)
