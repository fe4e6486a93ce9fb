"""GPU tests of the loss-scaled optimizer step: immtsf_adam_prepare_scaled / immtsf_adam_range_scaled / immtsf_loss_scale_update straight
through immtsf._lib, immtsf.optim.FusedAdam under torch.amp.GradScaler as main.py --use_amp writes the loop (main.py:1080-1091), and the
drop-in seam under torch.autocast and a scaled loss.

The kernels are compared ELEMENT BY ELEMENT with tests/amp_ref.py (pinned to torch on the CPU by tests/test_amp_ref.py) on the bars of
tests/test_gpu_optimizer.py: |got - ref| <= K 2^-24 Y with the yardsticks and K = 13 of oracle/optimizer_ref.py -- the scaled step adds
two multiplications to that update, one of them by a power of two, and K carries a factor 4 over a float32 emulation.  Buffers sit
between sentinels (test_gpu_optimizer.Guarded), checked after every call."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import amp_ref as A  # noqa: E402
import test_gpu_optimizer as TO  # noqa: E402
from oracle import optimizer_ref as R  # noqa: E402

SCRATCH = 2056
COEF, INV, SKIP, TICKET = 2048, 2049, 2050, 2051
NS = (1, 7, 8, 8 * 1024 + 3)
SCALES = (None, 1.0, 65536.0, 1000.0)
MAX_NORMS = (1.0, 1e12, 0.0)           # clip active (every gradient below has ||S g|| >= 3.7), inactive, off
WD = 1e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class State(TO.State):
    """test_gpu_optimizer.State with the scratch of the scaled entry points and the device floats they read and write"""

    def __init__(self, dev, n, offset=0):
        super().__init__(dev, n, offset)
        self.scratch = TO.Guarded(dev, SCRATCH)
        self.scale, self.fin, self.fout = (TO.Guarded(dev, 1) for _ in range(3))
        self.all = [self.p, self.g, self.m, self.v, self.scratch, self.step, self.drop, self.skip, self.scale, self.fin, self.fout]

    def load(self, init, step0, scale=None, found_in=0.0):
        super().load(init, step0)
        self.scratch.t.fill_(float("nan"))
        self.scratch.t[TICKET:].zero_()             # the ticket is zero between calls; everything in front of it is written
        self.scale.t.fill_(1.0 if scale is None else scale)
        self.fin.t.fill_(found_in)
        self.fout.t.fill_(0.0)


def _prepare(B, L, S, max_norm, scale, found_in=False):
    B.check(L.immtsf_adam_prepare_scaled(S.g.ptr, None, S.n, S.scratch.ptr, S.step.ptr, S.drop.ptr, None, None, None, None, S.skip.ptr,
                                         None if scale is None else S.scale.ptr, S.fin.ptr if found_in else None, S.fout.ptr, max_norm,
                                         B.stream_ptr()), "adam_prepare_scaled")


def _ranges(B, L, S, pieces, zero=1):
    for lo, hi in pieces:
        B.check(L.immtsf_adam_range_scaled(S.p.ptr, S.g.ptr, None, S.m.ptr, S.v.ptr, S.n, lo, hi, R.LR, R.B1, R.B2, R.EPS, WD, S.step.ptr,
                                           S.scratch.ptr, zero, None, B.stream_ptr()), "adam_range_scaled")


def _case(n, scale, step):
    """fp32 (p, g as stored, m, v): magnitudes over four decades, the true gradient normalised to ||g|| = 3.7 so that max_norm = 1
    clips at every scale, then stored times the scale (rounded to fp32: the stored gradient IS the input); m = v = 0 at step 1"""
    rng = np.random.default_rng([n, step, 0 if scale is None else int(scale)])
    mag = 10.0 ** rng.uniform(-3.0, 1.0, n)
    g = mag * np.copysign(np.maximum(np.abs(rng.standard_normal(n)), 2.0 ** -4), rng.standard_normal(n))
    g *= 3.7 / np.sqrt(np.dot(g, g))
    gs = (g * (1.0 if scale is None else scale)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    m = (mag * rng.standard_normal(n)).astype(np.float32)
    v = ((mag * rng.standard_normal(n)) ** 2).astype(np.float32)
    if step == 1:
        m, v = np.zeros_like(m), np.zeros_like(v)
    return p, gs, m, v


def _reference(case, scale, max_norm, step):
    """amp_ref's values with the ABI's fp32 hyperparameters, and the yardsticks of oracle/optimizer_ref for the same update (the
    unscaled gradient g inv with the norm of the stored one; tests/test_amp_ref.py holds the two to 1e-13 of each other)"""
    p, gs, m, v = case
    a = A.scaled_step(p, gs, m, v, step - 1, lr=R.f32(R.LR), b1=R.f32(R.B1), b2=R.f32(R.B2), eps=R.f32(R.EPS), wd=R.f32(WD),
                      max_norm=R.f32(max_norm), scale=scale, clip_eps=R.f32(1e-6))
    y = R.clip_adam_f64(p.astype(np.float64), gs.astype(np.float64) * A.inv_scale(scale), m, v, R.LR, R.B1, R.B2, R.EPS, WD, step, max_norm,
                        norm_sq=a.norm_sq)
    return a, y._replace(p=a.p, m=a.m, v=a.v)


class _Partials:
    """the view of a State that test_gpu_optimizer._check_partials sums: the 1024 partials alone"""

    def __init__(self, S):
        self.scratch = type("V", (), {"t": S.scratch.t[:1024]})()


@pytest.mark.parametrize("n", NS)
def test_scaled_step_against_float64(n):
    dev = _dev()
    B, L = TO._lib()
    S = State(dev, n)
    pieces_all = [[(0, n)]] + ([[(8, n), (0, 8)]] if n > 8 else [])
    worst = [0.0, 0.0, 0.0]
    for scale in SCALES:
        for step in (1, 3):
            case = _case(n, scale, step)
            init = [torch.from_numpy(a).to(dev) for a in case]
            for max_norm in MAX_NORMS:
                a, y = _reference(case, scale, max_norm, step)
                assert (a.coef < 0.5) == (max_norm == 1.0)
                D = TO.DevRef(y, dev)
                for pieces in pieces_all:
                    what = f"n={n} S={scale} max_norm={max_norm} step={step} pieces={pieces}"
                    S.load(init, step - 1, scale)
                    _prepare(B, L, S, max_norm, scale)
                    _ranges(B, L, S, pieces)
                    rs = (TO._ratio(S.p.t, D.p, D.Yp), TO._ratio(S.m.t, D.m, D.Ym), TO._ratio(S.v.t, D.v, D.Yv))
                    worst = [max(w, r) for w, r in zip(worst, rs)]
                    assert all(r <= R.K for r in rs), (what, "ratio to the yardstick (p, m, v)", rs, "K", R.K)
                    TO._check_partials(_Partials(S), a.norm_sq, n, what)
                    TO._check_side_effects(S, init, True, True, step, what)
                    sc = S.scratch.t
                    assert int(S.skip.t[0]) == 0 and float(S.fout.t[0]) == 0.0, what
                    assert int(sc[SKIP:SKIP + 1].view(torch.int32)[0]) == 0 and int(sc[TICKET:TICKET + 1].view(torch.int32)[0]) == 0, what
                    assert float(sc[INV]) == A.inv_scale(scale), (what, float(sc[INV]))
                    assert abs(float(sc[COEF]) - a.coef) <= (y.c_n + 1) * 2.0 ** -23 * a.coef, (what, float(sc[COEF]), a.coef)
    print(f"n={n}: worst |got - ref| / (2^-24 Y) (p, m, v) = {worst}, K = {R.K}")


@pytest.mark.parametrize("n", NS)
def test_without_a_scale_it_is_adam_range_bit_for_bit(n):
    """grad_scale NULL, finite gradient: immtsf_adam_prepare_scaled + _range_scaled leave the bits immtsf_adam_prepare + _range leave --
    parameters, moments, the 1024 partials, the counters"""
    dev = _dev()
    B, L = TO._lib()
    Sa, Sb = TO.State(dev, n), State(dev, n)
    pieces = [(0, 8), (8, n)] if n > 8 else [(0, n)]
    for step in (1, 3):
        for max_norm in MAX_NORMS:
            init = [torch.from_numpy(a).to(dev) for a in _case(n, None, step)]
            Sa.load(init, step - 1)
            TO.r_range(B, L, Sa, dict(lr=R.LR, b1=R.B1, b2=R.B2, eps=R.EPS, wd=WD, mn=max_norm), step, pieces=pieces)
            Sb.load(init, step - 1)
            _prepare(B, L, Sb, max_norm, None)
            _ranges(B, L, Sb, pieces)
            for name in ("p", "m", "v", "g", "step", "drop"):
                assert torch.equal(getattr(Sa, name).b, getattr(Sb, name).b), (n, step, max_norm, name)
            assert torch.equal(Sa.scratch.b, Sb.scratch.b[:1024]), (n, step, max_norm, "partials")
            assert Sa.intact() and Sb.intact()


@pytest.mark.parametrize("n", [7, 8 * 1024 + 3])
def test_skipped_steps_change_nothing_but_the_zero_fill(n):
    dev = _dev()
    B, L = TO._lib()
    S = State(dev, n)
    cases = {"found_inf_in": (None, None), "nan at 0": (0, float("nan")), "+inf at n-1": (n - 1, float("inf")),
             "-inf mid-buffer": (n // 2, float("-inf"))}
    for scale in (None, 65536.0):
        for name, (at, val) in cases.items():
            p, gs, m, v = _case(n, scale, 3)
            if at is not None:
                gs = gs.copy()
                gs[at] = val
            init = [torch.from_numpy(a).to(dev) for a in (p, gs, m, v)]
            S.load(init, 2, scale, found_in=1.0 if at is None else 0.0)
            _prepare(B, L, S, 1.0, scale, found_in=True)
            _ranges(B, L, S, [(0, 8), (8, n)] if n > 8 else [(0, n)])
            what = (n, scale, name)
            for key, src in (("p", init[0]), ("m", init[2]), ("v", init[3])):
                assert torch.equal(getattr(S, key).b, src.view(torch.int32)), (what, key, "changed on a skipped step")
            assert bool((S.g.b == 0).all()), (what, "grad not left zero")
            assert int(S.step.t[0]) == 2 and int(S.drop.t[0]) == 42, (what, int(S.step.t[0]), int(S.drop.t[0]))
            assert int(S.skip.t[0]) == 1 and float(S.fout.t[0]) == 1.0, (what, int(S.skip.t[0]), float(S.fout.t[0]))
            assert int(S.scratch.t[TICKET:TICKET + 1].view(torch.int32)[0]) == 0, what
            assert S.intact(), what


def test_loss_scale_update_follows_the_pinned_pattern():
    dev = _dev()
    B, L = TO._lib()
    scale, tracker, found = TO.Guarded(dev, 1), TO.Guarded(dev, 1, torch.int32), TO.Guarded(dev, 1)
    scale.t.fill_(A.PATTERN_INIT)
    tracker.t.fill_(0)
    got = []
    for f in A.PATTERN_FOUND:
        found.t.fill_(1.0 if f else 0.0)
        B.check(L.immtsf_loss_scale_update(scale.ptr, tracker.ptr, found.ptr, 2.0, 0.5, A.PATTERN_INTERVAL, B.stream_ptr()), "loss_scale_update")
        got.append((float(scale.t[0]), int(tracker.t[0])))
    assert got == A.pattern_scales()
    assert scale.intact() and tracker.intact() and found.intact()
    scale.t.fill_(float(np.finfo(np.float32).max))          # growth that would reach inf is not taken
    tracker.t.fill_(2)
    B.check(L.immtsf_loss_scale_update(scale.ptr, tracker.ptr, found.ptr, 2.0, 0.5, 3, B.stream_ptr()), "loss_scale_update")
    assert (float(scale.t[0]), int(tracker.t[0])) == (float(np.finfo(np.float32).max), 0)


# ---- the loop as main.py writes it ---------------------------------------------------------------------------------------------------

SHAPES = ((5, 3), (8,), (37,), (4, 4))          # unequal sizes, 15 and 37 are no multiples of 8
LOOP_STEPS, LOOP_INF_AT = 8, 3


def _loop(dev, fused, unscale_first, amp=True, guard=None):
    """eight steps of main.py's --use_amp loop on a small least-squares problem with weight decay (Adam alone is nearly blind to the
    gradient's scale: weight decay and eps are what make the clip order visible); an inf is written into one gradient at step 3"""
    from immtsf import config, optim
    old = config.optim_amp
    config.optim_amp = amp
    try:
        gen = torch.Generator().manual_seed(5)
        params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(dev)) for s in SHAPES]
        xs = [(0.05 * torch.randn(LOOP_STEPS, *s, generator=gen)).to(dev) for s in SHAPES]
        mk = optim.Adam if fused else optim._torch_adam
        clip = optim.clip_grad_norm_ if fused else optim._torch_clip
        opt = mk(params, lr=1e-2, eps=1e-3, weight_decay=0.01)
        assert isinstance(opt, optim.FusedAdam) == fused
    finally:
        config.optim_amp = old
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0, growth_interval=3)
    items = 0
    for i in range(LOOP_STEPS):
        opt.zero_grad()
        loss = sum(((p * x[i]).sum() - 1.0) ** 2 for p, x in zip(params, xs))
        scaler.scale(loss).backward()
        if i == LOOP_INF_AT:
            params[2].grad[36] = float("inf")
        if unscale_first:
            scaler.unscale_(opt)
        clip(params, 1.0)
        if guard:
            # no host read between the backward and the next step: guard "error" makes a synchronising call raise where the runtime
            # honours the mode, and .item() -- what GradScaler's generic route reads found_inf with -- is counted under either guard
            real_item = torch.Tensor.item
            calls = []
            torch.Tensor.item = lambda self: (calls.append(1), real_item(self))[1]
            torch.cuda.set_sync_debug_mode("error" if guard == "error" else "default")
            try:
                scaler.step(opt)
                scaler.update()
            finally:
                torch.cuda.set_sync_debug_mode("default")
                torch.Tensor.item = real_item
            items += len(calls)
        else:
            scaler.step(opt)
            scaler.update()
    torch.cuda.synchronize()
    st = [opt.state[p] for p in params]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()      # noqa: E731
    return dict(p=flat(params), m=flat([s["exp_avg"] for s in st]), v=flat([s["exp_avg_sq"] for s in st]),
                step=int(float(st[0]["step"])), scale=float(scaler.get_scale()), tracker=int(scaler._growth_tracker), items=items)


def _same(a, b, tol=2e-4):
    """the bar of test_gpu_train.py::test_optim_shim_trains_like_torch_adam, on parameters and both moments"""
    for k in ("p", "m", "v"):
        assert float((a[k] - b[k]).abs().max() / b[k].abs().max()) < tol, k
    for k in ("step", "scale", "tracker"):
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("unscale_first", [False, True])
def test_fused_adam_under_grad_scaler_trains_like_torch(unscale_first):
    dev = _dev()
    ref = _loop(dev, False, unscale_first)
    got = _loop(dev, True, unscale_first, guard="error")
    # three clean steps double the scale, the inf at step 3 halves it and is not counted, three more clean steps double it again
    assert ref["step"] == LOOP_STEPS - 1 and ref["tracker"] == 1 and ref["scale"] == 131072.0
    _same(got, ref)
    assert got["items"] == 0, "scaler.step() / update() read a tensor on the host"


def test_optim_amp_off_is_the_generic_route():
    """config.optim_amp = False (IMMTSF_OPTIM_AMP=0): GradScaler unscales the gradients itself, reads found_inf on the host and then calls
    step(), whose deferred clip therefore sees the UNSCALED gradient.  That is what the loss-scale route computes when the caller unscales
    first -- and not what main.py's order means, which is why the route exists"""
    dev = _dev()
    generic = _loop(dev, True, False, amp=False, guard="count")
    assert generic["items"] > 0                                   # (the host read of the generic route: one per step)
    _same(generic, _loop(dev, True, True), tol=1e-6)
    main_py = _loop(dev, True, False)
    assert float((generic["m"] - main_py["m"]).abs().max() / main_py["m"].abs().max()) > 1e-2


# ---- the seam under autocast and a scaled loss -----------------------------------------------------------------------------------------

def test_seam_under_autocast_and_a_scaled_loss():
    """compute_all_losses inside torch.autocast is the call outside it, bit for bit; scaler.scale(loss).backward() with S = 2^16 leaves
    S times the unscaled gradients, at the first (eager) sighting of the batch shape, at the capturing one and at a replay"""
    dev = _dev()
    import test_gpu_train as TT
    from immtsf import config
    from lib import evaluation as ev
    from lib.evaluation import compute_all_losses
    old = config.seam_graph
    S = 65536.0
    try:
        ev._graphs.clear(); ev._seen.clear()
        config.seam_graph = False
        model, fusion, _, batch = TT._setup(dev, 0.0, trainer=False)
        params = [p for p in list(model.parameters()) + list(fusion.parameters())]
        plain = compute_all_losses(model, fusion, batch)["loss"]
        with torch.autocast("cuda"):
            cast = compute_all_losses(model, fusion, batch)["loss"]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            cast_bf = compute_all_losses(model, fusion, batch)["loss"]
        assert cast.dtype == torch.float32
        assert torch.equal(plain.detach().view(torch.int32), cast.detach().view(torch.int32))
        assert torch.equal(plain.detach().view(torch.int32), cast_bf.detach().view(torch.int32))
        plain.backward()
        g_ref = [None if p.grad is None else p.grad.clone() for p in params]
        scaler = torch.amp.GradScaler("cuda", init_scale=S)
        config.seam_graph = True
        for sighting in ("eager", "capture", "replay"):
            for p in params:
                p.grad = None
            with torch.autocast("cuda"):
                loss = compute_all_losses(model, fusion, batch)["loss"]
            scaler.scale(loss).backward()
            assert abs(float(loss.detach()) - float(plain.detach())) <= 1e-5 * abs(float(plain.detach())), sighting
            for p, a in zip(params, g_ref):
                assert (p.grad is None) == (a is None), sighting
                if a is not None:      # (1e-4: the gradient bar of test_gpu_train.py -- atomic sums of cancelling terms change order)
                    assert float((p.grad - S * a).abs().max()) <= 1e-4 * S * max(float(a.abs().max()), 1e-6), sighting
        assert sum(len(v) for v in ev._graphs.values()) == 1
    finally:
        config.seam_graph = old
        ev._graphs.clear(); ev._seen.clear()
