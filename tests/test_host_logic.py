"""Host-side logic of the round-5 additions, on the CPU (no kernel is called): the optimizer shim's routing (reference main.py:1024,
1098-1101), the registries that carry the fused tail's hand-over between the autograd ops, the guard against two writers of one
gradient sink."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def test_optim_shim_routes_cpu_and_unusual_arguments_to_torch():
    from immtsf import optim
    p = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.ones(4))]
    o = optim.Adam(p, lr=1e-2, weight_decay=1e-3)
    assert isinstance(o, optim._torch_adam) and not isinstance(o, optim.FusedAdam)          # CPU parameters: torch's Adam
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(foreach=True)):
        assert isinstance(optim.Adam(p, **kw), optim._torch_adam)
    groups = [{"params": [p[0]]}, {"params": [p[1]], "lr": 1e-4}]
    assert isinstance(optim.Adam(groups), optim._torch_adam)                                  # parameter groups: torch's Adam
    # the clip of parameters no FusedAdam owns is torch's clip: same norm, gradients scaled in place
    for q in p:
        q.grad = torch.full_like(q, 2.0)
    want = torch.linalg.vector_norm(torch.cat([q.grad.reshape(-1) for q in p]))
    got = optim.clip_grad_norm_(p, 1.0)
    assert torch.allclose(got, want)
    assert torch.allclose(torch.linalg.vector_norm(torch.cat([q.grad.reshape(-1) for q in p])), torch.tensor(1.0), atol=1e-5)


def test_optim_shim_install_is_idempotent_and_reversible():
    from immtsf import optim
    a0, c0 = torch.optim.Adam, torch.nn.utils.clip_grad_norm_
    was = optim._installed
    try:
        optim.uninstall()
        assert torch.optim.Adam is optim._torch_adam and torch.nn.utils.clip_grad_norm_ is optim._torch_clip
        optim.install()
        optim.install()
        assert torch.optim.Adam is optim.Adam and torch.nn.utils.clip_grad_norm_ is optim.clip_grad_norm_
        optim.uninstall()
        assert torch.optim.Adam is optim._torch_adam
    finally:
        if was:
            optim.install()
        else:
            torch.optim.Adam, torch.nn.utils.clip_grad_norm_ = a0, c0


def test_handover_registry_matches_storage_shape_and_version():
    from immtsf import ops
    reg = []
    t = torch.zeros(4, 3)
    ops._reg_put(reg, t, "payload")
    assert ops._reg_take(reg, t) == "payload"
    assert ops._reg_take(reg, t.view(3, 4)) is None                  # another shape over the same data: not the tensor that was registered
    assert ops._reg_take(reg, torch.zeros(4, 3)) is None             # other storage
    assert ops._reg_take(reg, None) is None
    assert ops._reg_take(reg, t.t()) is None                         # not contiguous
    t.add_(1.0)                                                      # written since: the entry no longer describes it
    assert ops._reg_take(reg, t) is None
    u = torch.ones(2)
    ops._reg_put(reg, u, 1)
    assert ops._reg_take(reg, u, pop=True) == 1 and ops._reg_take(reg, u) is None
    for i in range(ops._SHADOW_CAP + 3):                            # bounded: the oldest entries go
        ops._reg_put(reg, torch.zeros(1), i)
    assert len(reg) == ops._SHADOW_CAP


def test_two_writers_of_one_undeclared_sink_raise_on_the_host():
    from immtsf import _lib, ops
    p = torch.nn.Parameter(torch.zeros(5))
    q = torch.nn.Parameter(torch.zeros(5))
    ops._claim_sinks([p, None], [None, None], "a")                   # no sink: nothing to guard
    ops._claim_sinks([p], [None], "b")
    p._immtsf_grad_sink = torch.zeros(5)
    ops._claim_sinks([p], [p._immtsf_grad_sink], "a")
    ops._claim_sinks([p], [p._immtsf_grad_sink], "a")                # the same op again (next step): fine
    with pytest.raises(_lib.ImmtsfError, match="sink_shared"):
        ops._claim_sinks([p], [p._immtsf_grad_sink], "b")
    q._immtsf_grad_sink = torch.zeros(5)
    q._immtsf_grad_shared = True                                     # declared shared: every writer accumulates
    ops._claim_sinks([q], [q._immtsf_grad_sink], "a")
    ops._claim_sinks([q], [q._immtsf_grad_sink], "b")


def test_ops_keeps_every_recorded_name():
    """tests/golden/ops_names.txt records the names immtsf.ops offers its callers (the drop-in modules, train.py, the tools and the tests
    reach private ones too): the list of the commit before the repeated idioms were folded, less the seven that the folds merged
    (_shadow_put / _shadow_get into _reg_put / _reg_take; _dlinear_table, _dl_tables, _tm_tables into _pointer_table; _tm_layouts,
    _cru_layouts into _grad_layout) and the `annotations` artefact of the __future__ import.  A later split of the module into a package
    has to keep every one importable from here, and every Function, class and front end THE object of the module that defines it
    (immtsf.ops or a submodule of it; immtsf._lib for the structs, check, ptr, stream_ptr), not a copy that can go stale."""
    import importlib
    import types
    from immtsf import ops
    with open(os.path.join(ROOT, "tests", "golden", "ops_names.txt")) as f:
        names = f.read().split()
    assert len(names) == len(set(names)) == 177
    missing = [n for n in names if not hasattr(ops, n)]
    assert not missing, missing
    owned = [n for n in names if isinstance(getattr(ops, n), (type, types.FunctionType))]
    assert len(owned) >= 150, len(owned)
    for n in owned:
        obj = getattr(ops, n)
        home = obj.__module__
        assert home == "immtsf._lib" or home == "immtsf.ops" or home.startswith("immtsf.ops."), (n, home)
        assert getattr(importlib.import_module(home), n) is obj, n
    merged = ("_shadow_put", "_shadow_get", "_dlinear_table", "_dl_tables", "_tm_tables", "_tm_layouts", "_cru_layouts")
    assert not [n for n in merged if hasattr(ops, n)]              # one definition each: no second copy grows back unnoticed


def test_t2v_form_selection_is_a_host_decision():
    """immtsf_ttf_t2v_xattn_folded (no kernel, no GPU): which formulation of TTF_T2V_XAttn a cfg gets -- the folded form from 8192 padded
    note rows on inside its limits (N <= 64), its mix-first variant for longer windows in bf16 mode with one head (or form 3), the chain
    as written otherwise (form 1, fp32 with long windows, several heads with long windows).  include/immtsf.h immtsf_fusion_cfg.form."""
    import ctypes as C
    from immtsf import _lib
    from immtsf.ops import make_cfg
    lib = _lib.load()

    def folded(B, N, T, d_m, d, H, bf16, form):
        cfg = make_cfg(B, N, T, 0, d_m, d, H, 1 if bf16 else 0, True, 0.1, 0.0, 0, None)
        cfg.form = form
        return lib.immtsf_ttf_t2v_xattn_folded(C.byref(cfg))

    assert folded(64, 32, 32, 768, 768, 1, True, 0) == 0            # 2048 padded rows: below the fold's fixed cost
    assert folded(256, 32, 32, 768, 768, 1, True, 0) == 1           # 8192 rows: folded
    assert folded(64, 32, 32, 768, 768, 1, True, 2) == 1
    assert folded(256, 32, 32, 768, 768, 1, True, 1) == 0           # the chain on request
    assert folded(64, 4096, 32, 4096, 768, 1, True, 0) == 1         # cfg5: long windows, bf16, one head -> mix-first
    assert folded(64, 4096, 32, 4096, 768, 1, False, 0) == 0        # fp32 mode: the chain
    assert folded(64, 4096, 32, 4096, 768, 2, True, 0) == 0         # two heads: the chain
    assert folded(64, 4096, 33, 4096, 768, 1, True, 3) == 0         # T > 32: outside both folded forms
    assert folded(4, 16, 8, 64, 32, 1, True, 3) == 1                # form 3 at any N inside its limits
    assert folded(4, 16, 8, 64, 32, 1, True, 1) == 0


def test_step_plan_lives_for_one_step_only():
    """immtsf.step_plan: the hand-overs between a step engine and the ops.  A plan is uninstalled when the step raises, and the
    parameter-gradient work it holds goes with it (a later step never launches a closure over a failed step's buffers); a second plan
    cannot be installed over the first; the head's "dY is ready" flag is handed out once.  No kernel is called."""
    from immtsf import step_plan
    from immtsf.step_plan import StepPlan
    ran = []
    plan = StepPlan()
    with pytest.raises(ValueError):
        with step_plan.install(plan):
            assert step_plan.current() is plan
            with pytest.raises(RuntimeError):
                with step_plan.install(StepPlan()):
                    pass
            assert step_plan.current() is plan                   # (the refused install left the first one in place)
            plan.hold_params = True
            plan.defer_params(lambda: ran.append("stale"))
            raise ValueError("a backward raised")
    assert step_plan.current() is not plan
    plan.run_params()
    with step_plan.install(StepPlan()) as fresh:
        fresh.run_params()
    assert ran == []

    plan = StepPlan()
    plan.head_flag = 0x1000
    dY = torch.zeros(3)
    assert plan.take_head_flag(dY) == 0x1000
    assert plan.take_head_flag(torch.zeros(3)) is None
    assert plan.head_dy_ptr == dY.data_ptr()

    idle = step_plan.current()                                   # outside an engine: nothing is offered
    assert idle.take_head_flag(dY) is None and idle.arm_gate() is None and not idle.hold_params
    assert not idle.wgrad_open and idle.ttf_flag is None and idle.defer == 0 and idle.announce is None
    assert idle.fold(lambda stream: ran.append("fold")) is False and ran == []


_RANGES = [(0, 4), (4, 8), (8, 8), (8, 12), (20, 24)]       # bucket 2 is empty; bucket 4 is no neighbour of the others


def _announcer(**kw):
    from immtsf.announce import Announcer
    emitted = []

    def emit(k, lo, hi):
        emitted.append((k, lo, hi))
        return 1000 + 4 * k
    return Announcer(_RANGES, emit, **kw), emitted


def _spans(a):
    return [(g["lo"], g["hi"]) for g in a.segments]


def test_announcer_single_buckets_and_bursts():
    """immtsf.announce.Announcer: which buckets of a data-parallel FlagStep share a flag.  Host logic only (a fake emit)."""
    from immtsf import announce
    assert not hasattr(announce, "torch") and not hasattr(announce, "_lib")
    a, emitted = _announcer()
    a.announce(1)
    assert a.segments == [{"flag": 1000, "flags": [1000], "lo": 4, "hi": 8, "buckets": (1,), "branch": "T"}]
    a.announce(1)                                                # a second announcement adds nothing
    assert len(a.segments) == 1 and emitted == [(0, 4, 8)]

    for merge, want in ((True, [(0, 12)]), (False, [(0, 4), (4, 8), (8, 12)])):
        a, emitted = _announcer(merge_adjacent=merge)
        token = object()
        for i, bi in enumerate((0, 1)):
            a.announce(bi, (token, i, 3))
            assert merge == (emitted == [])                      # a burst emits nothing before its last member
        a.announce(3, (token, 2, 3))
        assert _spans(a) == want and [k for k, _, _ in emitted] == list(range(len(want)))
        if merge:
            assert a.segments[0]["buckets"] == (0, 1, 3) and a.segments[0]["branch"] == "TTT" and a.segments[0]["flags"] == [1000]
        else:
            assert [g["buckets"] for g in a.segments] == [(0,), (1,), (3,)]

    a, _ = _announcer()
    token = object()
    a.announce(0, (token, 0, 2))
    a.announce(4, (token, 1, 2))
    assert _spans(a) == [(0, 4), (20, 24)] and [g["flag"] for g in a.segments] == [1000, 1004]


def test_announcer_finish_leaves_no_bucket_behind():
    a, _ = _announcer()
    a.finish()                                                   # nothing announced: everything behind the join, as contiguous runs
    assert _spans(a) == [(0, 12), (20, 24)] and [g["branch"] for g in a.segments] == ["JJJ", "J"]
    assert [g["buckets"] for g in a.segments] == [(0, 1, 3), (4,)]            # (the empty bucket is in no segment)

    # a burst whose LAST member was announced before it: the burst never closes by itself -- finish() emits its other members
    a, _ = _announcer()
    a.branch = "B"
    a.announce(3)
    a.branch = "T"
    token = object()
    for i, bi in enumerate((0, 1, 3)):
        a.announce(bi, (token, i, 3))
    assert _spans(a) == [(8, 12)]
    a.finish()
    assert _spans(a) == [(8, 12), (0, 8), (20, 24)]
    held = sorted(b for g in a.segments for b in g["buckets"])
    assert held == [0, 1, 3, 4]                                  # every non-empty bucket in exactly one segment
    covered = sorted(_spans(a))
    assert all(x[1] <= y[0] for x, y in zip(covered, covered[1:]))            # disjoint ranges
    assert all(len(g["branch"]) == len(g["buckets"]) for g in a.segments)


def test_announcer_capacity_and_orders():
    from immtsf.announce import Announcer, merge_tail, static_order
    a = Announcer([(8 * i, 8 * i + 4) for i in range(30)], lambda k, lo, hi: 1000 + 4 * k)      # no two are neighbours
    for bi in range(24):
        a.announce(bi)
    assert len(a.segments) == 24
    with pytest.raises(RuntimeError):
        a.announce(24)                                           # the 25th segment
    a = Announcer([(0, 4), (8, 12)], lambda k, lo, hi: k, capacity=1)
    with pytest.raises(RuntimeError):
        a.finish()

    segs = [{"branch": b, "n": i} for i, b in enumerate(["J", "T", "B", "TT", "P", "T", "PP"])]
    assert [g["n"] for g in static_order(segs)] == [1, 3, 4, 6, 5, 2, 0]    # T's but the last, P's, T's last, B's, J's
    assert static_order([]) == []

    def seg(k, lo, hi, buckets, branch, done):
        return {"flag": 1000 + 4 * k, "flags": [1000 + 4 * k], "lo": lo, "hi": hi, "buckets": buckets, "branch": branch, "done_us": done}
    early, b, c, d = seg(0, 0, 4, (0,), "T", 100.0), seg(1, 12, 20, (3, 4), "PP", 390.0), seg(2, 4, 12, (1, 2), "TT", 400.0), seg(3, 20, 24, (5,), "J", 430.0)
    out = merge_tail([early, b, c, d], 60.0)
    assert out[0] is early and len(out) == 2                     # an earlier bucket keeps its own segment
    assert out[1] == {"flag": 1012, "flags": [1004, 1008, 1012], "lo": 4, "hi": 24, "buckets": (1, 2, 3, 4, 5), "branch": "TTPPJ", "done_us": 430.0}
    gap = [seg(0, 0, 4, (0,), "T", 400.0), seg(1, 8, 12, (2,), "T", 430.0)]
    assert merge_tail(gap, 60.0) == gap                          # a tail that is not one contiguous range is left alone
    assert merge_tail([early, d], 60.0) == [early, d]            # nothing finished near the last one


def test_step_plan_offering_is_scoped():
    from immtsf.step_plan import StepPlan
    plan = StepPlan()
    assert plan.timeout_ms == 50 and StepPlan(timeout_ms=20).timeout_ms == 20
    with plan.offering(defer=3, tail_flag=0x40):
        assert (plan.defer, plan.tail_flag, plan.hold_params) == (3, 0x40, False)
        with plan.offering(hold_params=True, defer=1):           # it nests
            assert (plan.defer, plan.tail_flag, plan.hold_params) == (1, 0x40, True)
        assert (plan.defer, plan.tail_flag, plan.hold_params) == (3, 0x40, False)
    assert (plan.defer, plan.tail_flag) == (0, None)
    with pytest.raises(ValueError):
        with plan.offering(wgrad_flags=[1, 2], gate=(8, 12)):
            assert plan.wgrad_open
            raise ValueError("a backward raised")
    assert plan.wgrad_flags == [] and plan.gate is None          # restored after an exception too
    with pytest.raises(AttributeError):
        with plan.offering(jobs=[1]):                            # held work is no offer
            pass
    with pytest.raises(AttributeError):
        with plan.offering(defer=2, no_such_offer=1):
            pass
    assert plan.defer == 0 and plan.jobs == []
