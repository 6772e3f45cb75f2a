"""The backward plan of EtaLoop.sample (etainv/plan.py) as data, CPU only: which layout runs at which step for every controller and switch, the
control flags, the LocalBlend flag, the cost per image, the coefficients, the layout table's own consistency -- and that the loop executes
exactly what the plan says."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import pnp_ref as pr

ETA = [[0.6, 0], [1, 0.7]]                       # the paper's schedule: eta == 0 at t < 600
FULL, KEEP, EXIT, PNP, PLAIN = "u_s,u_t,c_s,c_t", "u_t,c_s,c_t", "u_t,c_t,c_s", "u_s,u_t,c_t", "u_t,c_t"


def _ptp(S, cross_steps, self_replace=0.6, blend=True):
    """the host tables of PtpTables the plan reads: cross alpha non-zero for the first `cross_steps` steps"""
    return SimpleNamespace(cross_active=np.arange(S + 1) < cross_steps, self_lo=0, self_hi=int(S * self_replace), blend_alpha=object() if blend else None)


def _plan(S=50, B=2, L=64, eta=ETA, **kw):
    from etainv.pipeline import alphas_cumprod, eta_table
    from etainv.plan import plan_backward
    delta = 1000 // S
    return plan_backward(S, (np.arange(S) * delta)[::-1], eta_table(eta), alphas_cumprod(), delta, L, B, **kw)


def _col(plan, *names):
    return [tuple(getattr(s, n) for n in names) if len(names) > 1 else getattr(s, names[0]) for s in plan]


def test_pie_prompt_to_prompt_settings():
    from etainv.flops import exit_share
    B, L = 2, 64
    plan = _plan(ptp=_ptp(50, 20))
    assert _col(plan, "layout") == [FULL] * 20 + [EXIT] * 30 and _col(plan, "trace_layout") == [FULL] * 20 + [PLAIN] * 30
    assert _col(plan[:20], "edit", "replay", "first_row", "src_exit_block", "self_replace_active") == [(True, False, 0, 0, True)] * 20
    assert _col(plan[20:30], "edit", "replay", "first_row", "src_exit_block", "self_replace_active") == [(False, True, B, 12, True)] * 10
    assert _col(plan[30:], "edit", "replay", "first_row", "src_exit_block", "self_replace_active") == [(False, True, B, 9, False)] * 20
    assert all(isinstance(s.cost, float) for s in plan)
    cost = sum(_col(plan, "cost"))
    assert cost == pytest.approx(20 * 4 + 10 * (2 + exit_share(L, 12)) + 20 * (2 + exit_share(L, 9)), abs=1e-9)
    assert abs(50 + cost - 207.34) < 0.01                                                    # + the S cond rows of the forward pass


def test_switches():
    ptp = _ptp(50, 20)
    plan = _plan(ptp=ptp, src_exit=False)
    assert _col(plan[20:], "layout", "trace_layout", "first_row", "src_exit_block", "cost") == [(KEEP, KEEP, 2, 0, 3.0)] * 30
    plan = _plan(ptp=ptp, src_exit_9_only=True)
    assert _col(plan[20:30], "layout", "src_exit_block") == [(KEEP, 0)] * 10 and _col(plan[30:], "layout", "src_exit_block") == [(EXIT, 9)] * 20
    plan = _plan(ptp=ptp, skip_dead_source_rows=False)
    assert _col(plan, "layout", "replay", "first_row", "cost") == [(FULL, False, 0, 4.0)] * 50
    assert _col(plan, "edit") == [True] * 20 + [False] * 30                                 # (the identity cross edit is still skipped)


@pytest.mark.parametrize("env, want", [(None, (True, True, False)), ("ETAINV_NO_DEAD_ROW_SKIP", (False, False, False)),
                                       ("ETAINV_NO_SRC_EXIT", (True, False, False)), ("ETAINV_SRC_EXIT_9_ONLY", (True, True, True))])
def test_loop_attributes_the_plan_reads(monkeypatch, env, want):
    from etainv.pipeline import EtaLoop
    for name in ("ETAINV_NO_DEAD_ROW_SKIP", "ETAINV_NO_SRC_EXIT", "ETAINV_SRC_EXIT_9_ONLY"):
        monkeypatch.delenv(name, raising=False)
    if env:
        monkeypatch.setenv(env, "1")
    loop = EtaLoop(SimpleNamespace(L=8, lib=None), S=50, eta=ETA)
    assert (loop.skip_dead_source_rows, loop.src_exit, loop.src_exit_9_only) == want
    # a target_dirinv weight needs the source row's own update: all 50 steps are full, as with skip_dead_source_rows=False
    loop = EtaLoop(SimpleNamespace(L=8, lib=None), S=50, eta=ETA, target_dirinv=0.5)
    assert (loop.skip_dead_source_rows, loop.src_exit) == (False, False)
    plan = _plan(ptp=_ptp(50, 20), skip_dead_source_rows=loop.skip_dead_source_rows, src_exit=loop.src_exit)
    assert _col(plan, "layout", "replay", "cost") == [(FULL, False, 4.0)] * 50 and _col(plan, "edit") == [True] * 20 + [False] * 30


def test_no_coupling():
    from etainv.plan import LAYOUTS
    plan = _plan()
    assert _col(plan, "layout", "replay", "cost") == [(FULL, False, 4.0)] * 20 + [(PLAIN, True, 2.0)] * 30
    assert LAYOUTS[PLAIN].latents == ("tgt",) and not LAYOUTS[PLAIN].ctrl                    # n_lat = B, no control
    assert not any(s.edit or s.self_replace_active or s.masa_active or s.pnp_qk_active or s.pnp_conv_active or s.blend or s.first_row for s in plan)


@pytest.mark.parametrize("S", [50, 100])
def test_masactrl(S):
    plan = _plan(S=S, masactrl=(4, 10))
    assert _col(plan, "layout", "replay", "cost") == [(FULL, False, 4.0)] * S
    assert _col(plan, "masa_active") == [4 <= i < 50 for i in range(S)] and not any(_col(plan[50:], "masa_active"))


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("S", [5, 50])
def test_pnp(S, skip):
    from etainv.flops import pnp_step_rows
    from etainv.plan import LAYOUTS
    conv, qk = pr.windows(S)
    plan = _plan(S=S, pnp=(conv, qk), skip_dead_source_rows=skip)
    eta_zero = [s.eta == 0.0 for s in plan]
    assert any(eta_zero) and not all(eta_zero)
    assert [len(LAYOUTS[s.layout].roles) for s in plan] == pr.step_rows(S, eta_zero, skip)
    assert _col(plan, "cost") == [float(pnp_step_rows(i, 1, conv, qk, skip and z)) for i, z in enumerate(eta_zero)]
    assert _col(plan, "layout") == [PNP if (i < max(conv, qk) or not z or not skip) else PLAIN for i, z in enumerate(eta_zero)]
    assert _col(plan, "layout") == _col(plan, "trace_layout") and (PLAIN in _col(plan, "layout")) == skip
    assert _col(plan, "pnp_conv_active", "pnp_qk_active") == [(c, q) for c, q in pr.step_flags(S)] == [(i < conv, i < qk) for i in range(S)]
    assert _col(plan, "replay") == [skip and z for z in eta_zero]


def test_edit_live_in_a_dead_step():
    plan = _plan(eta=0.0, ptp=_ptp(50, 51))
    assert _col(plan, "layout", "trace_layout", "edit", "replay", "first_row", "src_exit_block", "cost") == [(KEEP, KEEP, True, True, 2, 0, 3.0)] * 50


@pytest.mark.parametrize("S", [50, 8])
def test_local_blend_flag(S):
    want = [(i + 1) > int(0.2 * S) for i in range(S)]
    assert _col(_plan(S=S, ptp=_ptp(S, S // 2)), "blend") == want and any(want) and not all(want)
    assert not any(_col(_plan(S=S, ptp=_ptp(S, S // 2, blend=False)), "blend"))
    assert not any(_col(_plan(S=S), "blend")) and not any(_col(_plan(S=S, pnp=pr.windows(S)), "blend"))


def test_layout_table_is_self_consistent():
    from etainv.plan import LAYOUTS
    assert list(LAYOUTS) == [FULL, KEEP, EXIT, PNP, PLAIN]
    for name, lay in LAYOUTS.items():
        assert ",".join(lay.roles) == name and set(lay.roles) <= {"u_s", "u_t", "c_s", "c_t"} and set(lay.latents) <= {"src", "tgt"}
        for r, role in enumerate(lay.roles):                                                 # UNet row group r reads latent group r % n_lat
            assert lay.latents[r % len(lay.latents)] == {"s": "src", "t": "tgt"}[role[-1]], (name, r)
        assert (lay.roles[lay.eu], lay.roles[lay.ec]) == ("u_t", "c_t")
        assert lay.roles[lay.n_out:] == (("c_s",) if name == EXIT else ())                   # rows without output: the exited c_s
        assert lay.ctrl == (name != PLAIN)
    # first_row is B for the two layouts that start with u_t under prompt-to-prompt, 0 everywhere else
    B = 3
    plans = [_plan(B=B, ptp=_ptp(50, 20)), _plan(B=B, ptp=_ptp(50, 20), src_exit=False), _plan(B=B), _plan(B=B, pnp=pr.windows(50)),
             _plan(B=B, masactrl=(4, 10))]
    seen = {(s.layout, s.first_row) for plan in plans for s in plan}
    assert seen == {(FULL, 0), (KEEP, B), (EXIT, B), (PNP, 0), (PLAIN, 0)}


@pytest.mark.parametrize("S", [8, 50])
def test_coefficients(S):
    from etainv.pipeline import alphas_cumprod, eta_table
    ac, etas, delta = alphas_cumprod(), eta_table(ETA), 1000 // S
    plan = _plan(S=S)
    assert _col(plan, "t") == [(S - 1 - i) * delta for i in range(S)]
    for s in plan:
        t = s.t
        p = t - delta
        a_t, a_p = float(ac[t]), (float(ac[p]) if p >= 0 else float(ac[0]))
        var = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        assert (s.a_t, s.a_p, s.var, s.eta) == (a_t, a_p, var, float(etas[t]))
        assert all(type(v) is float for v in (s.a_t, s.a_p, s.var, s.eta))


class _Lib:
    def __getattr__(self, name):
        return lambda *a, **k: 0


class _Recorder:
    L, lib, map_div = 8, _Lib(), 4

    def __init__(self):
        self.calls = []

    def unet(self, latent, t, ctx, ctrl=None, out=None):
        c = ctrl.c if ctrl is not None else None
        self.calls.append((ctx.shape[0], latent.shape[0], int(t), c.first_row if c else 0, c.src_exit_block if c else 0, bool(c.mapper) if c else False,
                           bool(c.self_replace_active) if c else False, bool(c.masa_active) if c else False, bool(c.pnp_qk_active) if c else False,
                           bool(c.pnp_conv_active) if c else False, c is not None))
        out.zero_()
        return out

    def maps_configure(self, div): self.map_div = div
    def maps_reset(self): pass
    def word_maps_ex(self, *a, **k): pass
    def local_blend(self, x, *a, **k): self.calls[-1] += ("blend",)

    @contextlib.contextmanager
    def cached_context(self):
        yield


def test_the_loop_executes_the_plan(monkeypatch):
    """the recorder engine of test_backward_loop_row_economy_host_logic: every UNet call of EtaLoop.sample is the plan's record"""
    from etainv import _capi
    from etainv.pipeline import EtaLoop, PtpTables
    from etainv.plan import LAYOUTS, plan_backward
    monkeypatch.setattr(_capi, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_capi, "stream_ptr", lambda: None)
    monkeypatch.setattr(_capi, "check", lambda rc: None)
    B, L = 2, 8

    def check(S, loop_kw=None, **kw):
        eng = _Recorder()
        loop = EtaLoop(eng, S=S, eta=ETA, **(loop_kw or {}))
        inv = {"latents": torch.zeros(S + 1, B, 4, L, L), "maps_mean": torch.zeros(B, 3, L, L), "maps_steps": None}
        ctx = torch.zeros(B, 2, 77, 768)
        loop.sample(inv, ctx, ctx, torch.zeros(S, 10, 4, L, L), edit_word=torch.ones(B, dtype=torch.int64), **kw)
        plan = plan_backward(S, loop.t_bwd, loop.etas, loop.ac, loop.delta, L, B, loop.skip_dead_source_rows, loop.src_exit, loop.src_exit_9_only,
                             kw.get("ptp"), kw.get("masactrl"), kw.get("pnp"))
        want = []
        for s in plan:
            lay = LAYOUTS[s.layout]
            on = lay.ctrl and bool(kw)
            want.append((len(lay.roles) * B, len(lay.latents) * B, s.t, s.first_row, s.src_exit_block, on and s.edit, on and s.self_replace_active,
                         on and s.masa_active, on and s.pnp_qk_active, on and s.pnp_conv_active, on) + (("blend",) if s.blend else ()))
        assert eng.calls == want and len(want) == S
        assert abs(loop.rows_executed - B * sum(s.cost for s in plan)) < 1e-9
        return plan
    S = 50
    ca = np.zeros((S + 1, B, 77), np.float32)
    ca[:20] = 1.0
    ptp = PtpTables(np.tile(np.arange(77, dtype=np.int32), (B, 1)), np.ones((B, 77), np.float32), ca, 0.6, S, equalizer=np.ones((B, 77), np.float32),
                    blend_alpha=np.zeros((B, 2, 77), np.float32), device="cpu")
    plan = check(S, ptp=ptp)                                                                  # item 1: the PIE settings
    assert _col(plan, "layout") == [FULL] * 20 + [EXIT] * 30 and any(_col(plan, "blend"))
    assert _col(check(S), "layout") == [FULL] * 20 + [PLAIN] * 30                             # item 3: no coupling
    for S, skip in ((5, True), (50, True), (50, False)):                                      # item 5: pnp
        plan = check(S, dict(use_mask=False, skip_dead_source_rows=skip), pnp=pr.windows(S))
        assert (PLAIN in _col(plan, "layout")) == skip
