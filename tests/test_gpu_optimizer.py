"""GPU tests of the optimizer tail (csrc/tail.hip): every entry point in front of adam_kernel -- immtsf_adam_step, _step_dev, _step_dev_zero,
_step_guarded, _sqnorm + _apply, _prepare + _range, immtsf_guard_pack -- and the two bf16 streams, called straight through immtsf._lib.

The update is compared ELEMENT BY ELEMENT with the float64 reference of oracle/optimizer_ref.py at the eps = 1e-8 main.py trains with:
|got - ref| <= K 2^-24 Y with the yardsticks Y and the constant K of that module (K = 4 x what a float32 emulation reaches; never taken
from a kernel).  Inputs are given, not computed, every comparison is ONE step from the device's own fp32 state, and no element is masked.
Every buffer is a view into a larger allocation with 64 sentinel elements on both sides, checked bit for bit after each call.  The bf16
streams and the twins are compared bit for bit with bf16_rne / bf16_widen."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import optimizer_ref as R  # noqa: E402

PAD = 64
SENT = {2: 0x5AA5, 4: 0x5AA55AA5, 8: 0x5AA55AA55AA55AA5}
BITS = {2: torch.int16, 4: torch.int32, 8: torch.int64}
GRID_PASS = 2048 * 256 * 4          # elements one pass of adam_kernel's grid-stride loop covers
SMALL = (1, 3, 4, 5, 255, 256, 1023, 1025, 4099)
LARGE = (2 ** 18 + 3, 2 * GRID_PASS + 7, 8 * 1024 * 1024 + 3)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _lib():
    from immtsf import _lib as B
    return B, B.load()


class Guarded:
    """n elements inside a larger allocation, 64 + `offset` sentinel elements in front (offset = 1: the view starts one element off
    its 16-byte boundary) and at least 64 behind"""

    def __init__(self, dev, n, dtype=torch.float32, offset=0):
        size = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.empty(PAD + offset + n + PAD + 8, dtype=dtype, device=dev)
        self.bits = self.raw.view(BITS[size])
        self.sent = SENT[size]
        self.bits.fill_(self.sent)
        self.lo, self.n = PAD + offset, n
        self.t = self.raw[self.lo:self.lo + n]
        self.b = self.bits[self.lo:self.lo + n]
        self.size, self.addr = size, self.raw.data_ptr() + self.lo * size      # (an empty view has no data_ptr of its own)
        assert (self.addr % 16 == 0) == (offset == 0)

    def intact(self):
        return bool((self.bits[:self.lo] == self.sent).all()) and bool((self.bits[self.lo + self.n:] == self.sent).all())

    @property
    def ptr(self):
        return C.c_void_p(self.addr)


def _at(g, elems):
    return C.c_void_p(g.addr + elems * g.size)


class State:
    """the flat buffers of one optimizer (p, g, m, v), the norm scratch, the device words, optionally a bf16 twin / a bf16 gradient wire"""

    def __init__(self, dev, n, offset=0, twin=None, wire=None):
        self.n, self.dev = n, dev
        self.p, self.g, self.m, self.v = (Guarded(dev, n, offset=offset) for _ in range(4))
        self.scratch = Guarded(dev, 1024)
        self.step, self.drop = Guarded(dev, 1, torch.int64), Guarded(dev, 1, torch.int64)
        self.skip = Guarded(dev, 1, torch.int32)
        self.twin = None if twin is None else Guarded(dev, n, torch.int16, offset=twin)
        self.wire = None if wire is None else Guarded(dev, n, torch.int16, offset=wire)
        self.all = [x for x in (self.p, self.g, self.m, self.v, self.scratch, self.step, self.drop, self.skip, self.twin, self.wire)
                    if x is not None]

    def load(self, init, step0, drop0=41):
        for dst, src in zip((self.p, self.g, self.m, self.v), init):
            dst.t.copy_(src)
        self.step.t.fill_(step0)
        self.drop.t.fill_(drop0)
        self.skip.t.fill_(0)
        self.scratch.t.fill_(float("nan"))
        if self.twin is not None:
            self.twin.t.fill_(0x1234)
        if self.wire is not None:
            self.wire.t.copy_(torch.from_numpy(R.bf16_rne(init[1].cpu().numpy()).view(np.int16)).to(self.dev))

    def intact(self):
        return all(x.intact() for x in self.all)


def _hp(wd, max_norm):
    return dict(lr=R.LR, b1=R.B1, b2=R.B2, eps=R.EPS, wd=wd, mn=max_norm)


def _partition(n, k):
    cuts = sorted({0, n} | {(n * i // k) // 8 * 8 for i in range(1, k)})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


# ---- the update routes: each leaves p, m, v (and the twin) updated; returns (gradient left zero?, device counters advanced?) ----

def r_step(B, L, S, h, t):
    B.check(L.immtsf_adam_step(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], t, h["mn"],
                               S.scratch.ptr, B.stream_ptr()), "adam_step")
    return False, False


def r_dev(B, L, S, h, t):
    B.check(L.immtsf_adam_step_dev(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], S.step.ptr,
                                   h["mn"], S.scratch.ptr, S.drop.ptr, B.stream_ptr()), "adam_step_dev")
    return False, True


def r_dev_zero(B, L, S, h, t):
    B.check(L.immtsf_adam_step_dev_zero(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], S.step.ptr,
                                        h["mn"], S.scratch.ptr, S.drop.ptr, B.stream_ptr()), "adam_step_dev_zero")
    return True, True


def r_guarded(B, L, S, h, t, zero=0):
    B.check(L.immtsf_adam_step_guarded(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], S.step.ptr,
                                       h["mn"], S.scratch.ptr, S.drop.ptr, S.skip.ptr, zero, B.stream_ptr()), "adam_step_guarded")
    return bool(zero), True


def r_split_host(B, L, S, h, t, twin=None):
    B.check(L.immtsf_adam_sqnorm(S.g.ptr, S.n, S.scratch.ptr, None, None, B.stream_ptr()), "adam_sqnorm")
    B.check(L.immtsf_adam_apply(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], t, None, h["mn"],
                                S.scratch.ptr, twin, B.stream_ptr()), "adam_apply")
    return False, False


def r_split_dev(B, L, S, h, t, twin=None):
    B.check(L.immtsf_adam_sqnorm(S.g.ptr, S.n, S.scratch.ptr, S.step.ptr, S.drop.ptr, B.stream_ptr()), "adam_sqnorm")
    B.check(L.immtsf_adam_apply(S.p.ptr, S.g.ptr, S.m.ptr, S.v.ptr, S.n, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 0, S.step.ptr, h["mn"],
                                S.scratch.ptr, twin, B.stream_ptr()), "adam_apply")
    return False, True


def r_range(B, L, S, h, t, pieces=3, reverse=False, zero=1, wire=False, prepare=True):
    gh = S.wire.ptr if wire else None
    if prepare:
        B.check(L.immtsf_adam_prepare(S.g.ptr, gh, S.n, S.scratch.ptr, S.step.ptr, S.drop.ptr, None, None, None, None, S.skip.ptr,
                                      B.stream_ptr()), "adam_prepare")
    parts = _partition(S.n, pieces) if isinstance(pieces, int) else pieces
    for lo, hi in (parts[::-1] if reverse else parts):
        B.check(L.immtsf_adam_range(S.p.ptr, S.g.ptr, gh, S.m.ptr, S.v.ptr, S.n, lo, hi, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                                    S.step.ptr, h["mn"], S.scratch.ptr, zero, S.skip.ptr, B.stream_ptr()), "adam_range")
    return bool(zero), True


ROUTES = {"adam_step": r_step, "adam_step_dev": r_dev, "adam_step_dev_zero": r_dev_zero, "adam_step_guarded": r_guarded,
          "sqnorm+apply(step)": r_split_host, "sqnorm+apply(step_dev)": r_split_dev, "prepare+range": r_range}


# ---- comparison with the reference, on the device in float64 ----------------------------------------------------------------------

def _ratio(got, ref, Y):
    """max over all elements of |got - ref| / (2^-24 Y); a zero yardstick demands equality; NaN propagates (and fails `<= K`)"""
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    inf = torch.full_like(err, float("inf"))
    r = torch.where(Y > 0, err / (R.U32 * Y), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(r.max())


class DevRef:
    def __init__(self, ref, dev, sl=slice(None)):
        self.p, self.m, self.v, self.Yp, self.Ym, self.Yv = (torch.from_numpy(a[sl]).to(dev) for a in
                                                             (ref.p, ref.m, ref.v, ref.Yp, ref.Ym, ref.Yv))
        self.norm_sq, self.coef = ref.norm_sq, ref.coef


def _check_update(S, D, what, worst, sl=slice(None)):
    """p, m, v of the state (elements `sl`) against the reference: EVERY element within K yardsticks"""
    rs = (_ratio(S.p.t[sl], D.p, D.Yp), _ratio(S.m.t[sl], D.m, D.Ym), _ratio(S.v.t[sl], D.v, D.Yv))
    w = worst.setdefault(what, [0.0, 0.0, 0.0])
    for i, r in enumerate(rs):
        w[i] = max(w[i], r) if r == r else float("nan")
    assert all(r <= R.K for r in rs), (what, "ratio to the yardstick (p, m, v)", rs, "K", R.K)


def _check_partials(S, norm_sq, n, what, worst=None):
    """the 1024 partials, summed in float64, against ||g||^2 within the derived depth: all terms positive, one relative rounding each"""
    got = float(S.scratch.t.double().sum())
    bound = 1.001 * R.partials_depth(n) * R.U32 * norm_sq
    if worst is not None and norm_sq > 0:
        worst[0] = max(worst[0], abs(got - norm_sq) / (R.U32 * norm_sq))
    assert abs(got - norm_sq) <= bound, (what, got, norm_sq, abs(got - norm_sq) / max(norm_sq, 1e-300) / R.U32, R.partials_depth(n))


def _check_side_effects(S, init, zeroed, counted, t, what, drop0=41):
    assert S.intact(), (what, "a sentinel next to a buffer was overwritten")
    if zeroed:
        assert bool((S.g.b == 0).all()), (what, "grad not left exactly zero")
    else:
        assert torch.equal(S.g.b, init[1].view(torch.int32)), (what, "grad was written")
    if counted:
        assert int(S.step.t[0]) == t and int(S.drop.t[0]) == drop0 + 1, (what, int(S.step.t[0]), int(S.drop.t[0]))
    else:
        assert int(S.step.t[0]) == t - 1 and int(S.drop.t[0]) == drop0, (what, "host-step route touched the device counters")


def _prefetched(fn, items, depth=4):
    """fn over items on a few host threads, at most `depth` results alive ahead of the consumer (the float64 reference of 8 Mi elements
    is a second of numpy and half a gigabyte)"""
    items = list(items)
    with ThreadPoolExecutor(max_workers=depth) as ex:
        futs = [ex.submit(fn, it) for it in items[:depth]]
        for i, it in enumerate(items):
            res = futs[i].result()
            futs[i] = None
            if i + depth < len(items):
                futs.append(ex.submit(fn, items[i + depth]))
            yield it, res


def _member(base, member):
    wd, max_norm, step = member
    case = R.family_case(base, wd, max_norm, step)
    return case, R.clip_adam_f64(*case, R.LR, R.B1, R.B2, R.EPS, wd, step, max_norm)


# ---- a. the step against float64: six routes x the family x lengths x alignments ---------------------------------------------------

@pytest.mark.parametrize("n", SMALL + LARGE)
def test_step_against_float64(n):
    dev = _dev()
    B, L = _lib()
    base = R.family_base(n, 0)
    states = {"aligned": State(dev, n, 0), "one float in": State(dev, n, 1)}
    worst, worst_part = {}, [0.0]
    for member, (case, ref) in _prefetched(lambda mb: _member(base, mb), R.family()):
        wd, max_norm, t = member
        init = [torch.from_numpy(a).to(dev) for a in case]
        D = DevRef(ref, dev)
        del ref
        for al, S in states.items():
            for name, route in ROUTES.items():
                what = f"{name} n={n} {al} wd={wd} max_norm={max_norm} step={t}"
                S.load(init, t - 1)
                zeroed, counted = route(B, L, S, _hp(wd, max_norm), t)
                _check_update(S, D, name, worst)
                _check_partials(S, D.norm_sq, n, what, worst_part)
                _check_side_effects(S, init, zeroed, counted, t, what)
    print(f"n={n}: worst |got - ref| / (2^-24 Y) per route (p, m, v), K = {R.K}:")
    for name, w in worst.items():
        print(f"    {name:24s} p {w[0]:.3f}  m {w[1]:.3f}  v {w[2]:.3f}")
    print(f"    1024 partials vs ||g||^2: worst {worst_part[0]:.3f} roundings of {R.partials_depth(n)} allowed")


def test_clip_denominator_carries_1e_minus_6():
    """||g|| ~ 1e-5 against max_norm = 1e-6: the + 1e-6 of clip_grad_norm_ is a tenth of the coefficient here (at norms >> 1e-6 it is below
    the resolution of any fp32 comparison)"""
    dev = _dev()
    B, L = _lib()
    n = 1027
    rng = np.random.default_rng(11)
    z = rng.standard_normal(n)
    g = (1e-5 / np.sqrt(n) * np.copysign(np.maximum(np.abs(z), 2.0 ** -4), z)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    worst = {}
    for t in (1, 10):
        m = np.zeros(n, np.float32) if t == 1 else (g * rng.standard_normal(n)).astype(np.float32)
        v = np.zeros(n, np.float32) if t == 1 else (g * rng.standard_normal(n)).astype(np.float32) ** 2
        ref = R.clip_adam_f64(p, g, m, v, R.LR, R.B1, R.B2, R.EPS, 0.0, t, 1e-6, track_min=True)
        assert 0.05 < ref.coef < 0.2 and ref.min_nonzero >= R.MIN_INTERMEDIATE
        init = [torch.from_numpy(a).to(dev) for a in (p, g, m, v)]
        D = DevRef(ref, dev)
        for off in (0, 1):
            S = State(dev, n, off)
            for name, route in ROUTES.items():
                S.load(init, t - 1)
                zeroed, counted = route(B, L, S, _hp(0.0, 1e-6), t)
                _check_update(S, D, name, worst)
                _check_side_effects(S, init, zeroed, counted, t, f"{name} step={t} offset={off}")
    print("tiny norm: worst ratio per route (p, m, v):", {k: [round(x, 3) for x in w] for k, w in worst.items()})


# ---- b. routes that run the same kernel on the same arguments agree bit for bit -----------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [5, 1025, 4099, 2 ** 18 + 3])
def test_device_step_routes_agree_bit_for_bit(n, offset):
    """adam_step_dev, _dev_zero, _guarded(skip 0), sqnorm + apply(step_dev) and prepare + range launch adam_kernel with the same scalars,
    the same 1024 partials (both norm kernels stride the buffer alike) and the bias corrections of the same device powf; an element's
    arithmetic does not depend on the grid, on the piece it falls into or on the vector / scalar path.  (adam_step takes its bias
    corrections from the host's powf: not expected equal, and compared with the reference instead.)"""
    dev = _dev()
    B, L = _lib()
    base = R.family_base(n, 1)
    S = State(dev, n, offset)
    same = [("adam_step_dev_zero", r_dev_zero, {}), ("adam_step_guarded", r_guarded, {}), ("adam_step_guarded zero", r_guarded, {"zero": 1}),
            ("sqnorm+apply(step_dev)", r_split_dev, {})]
    for k in (1, 2, 5):
        for rev in (False, True):
            same.append((f"prepare+range {k} pieces{' reversed' if rev else ''}", r_range, {"pieces": k, "reverse": rev, "zero": k % 2}))
    for wd, max_norm, t in ((1e-3, 1.0, 1), (1e-3, 1.0, 10), (0.0, 1e9, 2), (0.0, 0.0, 1000)):
        init = [torch.from_numpy(a).to(dev) for a in R.family_case(base, wd, max_norm, t)]
        S.load(init, t - 1)
        r_dev(B, L, S, _hp(wd, max_norm), t)
        want = [x.b.clone() for x in (S.p, S.m, S.v)]
        assert not torch.equal(want[0], init[0].view(torch.int32))
        for name, route, kw in same:
            S.load(init, t - 1)
            route(B, L, S, _hp(wd, max_norm), t, **kw)
            for x, w, which in zip((S.p, S.m, S.v), want, "pmv"):
                assert torch.equal(x.b, w), (name, which, n, offset, wd, max_norm, t, int((x.b != w).sum()))
            assert S.intact(), name


# ---- c. the sharded form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cut", [2056, 1027])
def test_sharded_sqnorm_allreduce_apply(cut):
    """two shards of one buffer, each with its own adam_sqnorm; the partials are added on the device as the all-reduce would; adam_apply
    on each shard pointer with twin = NULL, so the SECOND shard's twin comes out of the registry at an offset into the registered range
    (cut = 1027: that shard and its twin are misaligned -- the scalar path)"""
    dev = _dev()
    B, L = _lib()
    n = 4099
    base = R.family_base(n, 2)
    S = State(dev, n, 0, twin=0)
    scr2 = Guarded(dev, 1024)
    worst = {}
    B.check(L.immtsf_bf16_twin_register(S.p.ptr, S.twin.ptr, n), "twin_register")
    try:
        for wd, max_norm, t in ((1e-3, 1.0, 3), (0.0, 1.0, 1), (1e-3, 1e9, 1000)):
            case = R.family_case(base, wd, max_norm, t)
            whole = R.clip_adam_f64(*case, R.LR, R.B1, R.B2, R.EPS, wd, t, max_norm)
            init = [torch.from_numpy(a).to(dev) for a in case]
            h = _hp(wd, max_norm)
            for use_dev_step in (False, True):
                S.load(init, t - 1)
                B.check(L.immtsf_adam_sqnorm(S.g.ptr, cut, S.scratch.ptr, S.step.ptr if use_dev_step else None,
                                             S.drop.ptr if use_dev_step else None, B.stream_ptr()), "adam_sqnorm")
                B.check(L.immtsf_adam_sqnorm(_at(S.g, cut), n - cut, scr2.ptr, None, None, B.stream_ptr()), "adam_sqnorm")
                S.scratch.t.add_(scr2.t)
                _check_partials(S, whole.norm_sq, n, "sharded")
                for lo, k in ((0, cut), (cut, n - cut)):
                    B.check(L.immtsf_adam_apply(_at(S.p, lo), _at(S.g, lo), _at(S.m, lo), _at(S.v, lo), k, h["lr"], h["b1"], h["b2"],
                                                h["eps"], h["wd"], 0 if use_dev_step else t, S.step.ptr if use_dev_step else None, h["mn"],
                                                S.scratch.ptr, None, B.stream_ptr()), "adam_apply")
                _check_update(S, DevRef(whole, dev), f"sharded cut={cut} step_dev={use_dev_step}", worst)
                _check_side_effects(S, init, False, use_dev_step, t, "sharded")
                assert scr2.intact()
                want = torch.from_numpy(R.bf16_rne(S.p.t.cpu().numpy()).view(np.int16)).to(dev)
                assert torch.equal(S.twin.t, want), ("twin of the shards", cut, int((S.twin.t != want).sum()))
    finally:
        L.immtsf_bf16_twin_unregister(S.p.ptr)
    print("sharded: worst ratio (p, m, v):", {k: [round(x, 3) for x in w] for k, w in worst.items()})


# ---- d. the bf16 streams, bit exact --------------------------------------------------------------------------------------------------

STREAM_LENGTHS = (0, 1, 3, 4, 5, 1027, 4096 * 256 * 4 + 5)


def _tiled(a, n, start):
    idx = (np.arange(n, dtype=np.int64) + start) % a.size
    return a[idx]


@pytest.mark.parametrize("n", STREAM_LENGTHS)
def test_f32_to_bf16_is_round_to_nearest_even(n):
    """all 65 536 high halves x the six low halves that decide the rounding (oracle.optimizer_ref.bf16_sweep), through the vector path,
    its tail, and -- source or destination one element off -- the scalar path.  Short lengths take windows of the sweep that start on a tie
    that carries into the exponent, on the overflow to inf and in front of the NaNs; the last length holds the whole sweep ten times over, so every pattern meets both paths."""
    dev = _dev()
    B, L = _lib()
    sweep = R.bf16_sweep()
    starts = (3 * 65536 + 0x3F7F, 3 * 65536 + 0x7F7E, 5 * 65536 + 0xFF7E) if n < sweep.size else (0, 7)
    for start in starts:
        x = _tiled(sweep, n, start)
        want = R.bf16_rne(x)
        nan = np.isnan(x)
        for so in (0, 1):
            for do in (0, 1):
                src, dst = Guarded(dev, n, offset=so), Guarded(dev, n, torch.int16, offset=do)
                src.b.copy_(torch.from_numpy(x.view(np.int32)).to(dev))
                rc = L.immtsf_f32_to_bf16(src.ptr, dst.ptr, n, B.stream_ptr())
                B.check(rc, "f32_to_bf16")
                got = dst.t.cpu().numpy().view(np.uint16)
                assert src.intact() and dst.intact(), (n, so, do)
                bad = np.flatnonzero(got[~nan] != want[~nan])
                assert bad.size == 0, (n, so, do, bad.size, [hex(int(v)) for v in x[~nan][bad[:4]].view(np.uint32)],
                                       [hex(int(v)) for v in got[~nan][bad[:4]]], [hex(int(v)) for v in want[~nan][bad[:4]]])
                assert np.isnan(R.bf16_widen(got[nan])).all(), (n, so, do, "a NaN did not stay NaN")


@pytest.mark.parametrize("n", STREAM_LENGTHS)
def test_bf16_to_f32_is_exact(n):
    dev = _dev()
    B, L = _lib()
    every = np.arange(65536, dtype=np.uint16)
    for start in ((0, 0x7F7E, 0xFF7E) if n < 65536 else (0, 3)):
        h = _tiled(every, n, start)
        want = R.bf16_widen(h).view(np.uint32)
        for so in (0, 1):
            for do in (0, 1):
                src, dst = Guarded(dev, n, torch.int16, offset=so), Guarded(dev, n, offset=do)
                src.t.copy_(torch.from_numpy(h.view(np.int16)).to(dev))
                B.check(L.immtsf_bf16_to_f32(src.ptr, dst.ptr, n, B.stream_ptr()), "bf16_to_f32")
                got = dst.b.cpu().numpy().view(np.uint32)
                assert src.intact() and dst.intact(), (n, so, do)
                nan = np.isnan(want.view(np.float32))
                assert np.array_equal(got[~nan], want[~nan]), (n, so, do)
                assert np.isnan(got.view(np.float32)[nan]).all(), (n, so, do)


# ---- e. twins and the wire -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twin_offset", [0, 1])
@pytest.mark.parametrize("n", [5, 1027, 4099])
def test_registered_twin_follows_every_route(n, twin_offset):
    """twin[lo:hi] = bf16_rne(new p) bit for bit after every route, the twin outside the updated range untouched; a misaligned twin sends
    the whole update down the scalar path, and the update itself stays within the yardsticks"""
    dev = _dev()
    B, L = _lib()
    base = R.family_base(n, 4)
    S = State(dev, n, 0, twin=twin_offset)
    wd, max_norm, t = 1e-3, 1.0, 3
    case, ref = _member(base, (wd, max_norm, t))
    init = [torch.from_numpy(a).to(dev) for a in case]
    D = DevRef(ref, dev)
    worst = {}
    sub = _partition(n, 3)[1:2] if n >= 24 else [(0, n)]
    routes = dict(ROUTES)
    routes["prepare+range, the middle piece only"] = lambda B_, L_, S_, h_, t_: r_range(B_, L_, S_, h_, t_, pieces=sub)
    B.check(L.immtsf_bf16_twin_register(S.p.ptr, S.twin.ptr, n), "twin_register")
    try:
        for name, route in routes.items():
            S.load(init, t - 1)
            zeroed, counted = route(B, L, S, _hp(wd, max_norm), t)
            lo, hi = sub[0] if "middle" in name else (0, n)
            assert S.intact(), name
            _check_update(S, DevRef(ref, dev, slice(lo, hi)) if (lo, hi) != (0, n) else D, name, worst, slice(lo, hi))
            got = S.twin.t.cpu().numpy().view(np.uint16)
            want = R.bf16_rne(S.p.t.cpu().numpy())
            assert np.array_equal(got[lo:hi], want[lo:hi]), (name, "twin != bf16_rne(p)", int((got[lo:hi] != want[lo:hi]).sum()))
            assert (got[:lo] == 0x1234).all() and (got[hi:] == 0x1234).all(), (name, "twin written outside the range")
            for x, src in ((S.p, init[0]), (S.m, init[2]), (S.v, init[3])):
                assert torch.equal(x.b[:lo], src.view(torch.int32)[:lo]) and torch.equal(x.b[hi:], src.view(torch.int32)[hi:]), name
            if zeroed:
                assert bool((S.g.b[lo:hi] == 0).all()) and torch.equal(S.g.b[:lo], init[1].view(torch.int32)[:lo]) and \
                    torch.equal(S.g.b[hi:], init[1].view(torch.int32)[hi:]), (name, "zero-fill is not exactly [lo, hi)")
    finally:
        L.immtsf_bf16_twin_unregister(S.p.ptr)
    # adam_apply with an explicit twin pointer (nothing registered)
    for name, route in (("apply(step) twin=", r_split_host), ("apply(step_dev) twin=", r_split_dev)):
        S.load(init, t - 1)
        route(B, L, S, _hp(wd, max_norm), t, twin=S.twin.ptr)
        assert S.intact(), name
        _check_update(S, D, name, worst)
        assert np.array_equal(S.twin.t.cpu().numpy().view(np.uint16), R.bf16_rne(S.p.t.cpu().numpy())), name
    # ... and without one the twin is nobody's business
    S.load(init, t - 1)
    r_dev(B, L, S, _hp(wd, max_norm), t)
    assert bool((S.twin.t == 0x1234).all())
    print(f"twins n={n} twin offset {twin_offset}: worst ratio (p, m, v):", {k: [round(x, 3) for x in w] for k, w in worst.items()})


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [5, 1027, 4099, 2 ** 18 + 3])
def test_bf16_gradient_wire(n, offset):
    """adam_prepare / adam_range reading grad_h = bf16_rne(grad): the reference takes the widened wire values as its gradient, so the same
    yardsticks hold; zero_grad still clears the fp32 grad; the fp32 grad is not read (it holds other numbers here)"""
    dev = _dev()
    B, L = _lib()
    base = R.family_base(n, 5)
    S = State(dev, n, offset, wire=offset)
    worst = {}
    for wd, max_norm, t in ((0.0, 1.0, 1), (1e-3, 1.0, 2), (1e-3, 1e9, 10), (0.0, 0.0, 100000)):
        p, g, m, v = R.family_case(base, wd, max_norm, t)
        gw = R.bf16_widen(R.bf16_rne(g))
        assert np.isfinite(gw).all()
        ref = R.clip_adam_f64(p, gw, m, v, R.LR, R.B1, R.B2, R.EPS, wd, t, max_norm)
        init = [torch.from_numpy(a).to(dev) for a in (p, g, m, v)]
        D = DevRef(ref, dev)
        for zero in (1, 0):
            S.load(init, t - 1)
            S.g.t.mul_(-3.0)
            kept = S.g.b.clone()
            r_range(B, L, S, _hp(wd, max_norm), t, pieces=3, zero=zero, wire=True)
            _check_update(S, D, f"wire zero_grad={zero}", worst)
            _check_partials(S, ref.norm_sq, n, "wire")
            assert S.intact()
            assert bool((S.g.b == 0).all()) if zero else torch.equal(S.g.b, kept)
            assert int(S.step.t[0]) == t and int(S.drop.t[0]) == 42
    print(f"wire n={n} offset {offset}: worst ratio (p, m, v):", {k: [round(x, 3) for x in w] for k, w in worst.items()})


# ---- f. the step decision and dropped steps --------------------------------------------------------------------------------------------

def test_prepare_decision_table():
    """*skip_out = (pending given and 0) | (err given and != 0) | (guard_h given and != 0) | (guard_f given and != 0); *pending cleared;
    *step_dev += 1 unless dropped; *dropout_step_dev += 1 always -- over the full table, NULL for every optional word included"""
    dev = _dev()
    B, L = _lib()
    n = 40
    S = State(dev, n, 0)
    base = R.family_base(n, 6)
    init = [torch.from_numpy(a).to(dev) for a in R.family_case(base, 0.0, 1.0, 3)]
    pending, err = Guarded(dev, 1, torch.int32), Guarded(dev, 1, torch.int32)
    gh, gf = Guarded(dev, 1, torch.int16), Guarded(dev, 1)
    bf = {0: 0x0000, 1: 0x3F80, 2: 0x4000}
    seen = 0
    for pv in (None, 0, 1):
        for ev in (None, 0, 7):
            for hv in (None, 0, 1, 2):
                for fv in (None, 0, 1, 2):
                    S.load(init, 5, drop0=9)
                    S.skip.t.fill_(-77)
                    pending.t.fill_(pv or 0)
                    err.t.fill_(ev or 0)
                    gh.t.fill_(bf[hv or 0])
                    gf.t.fill_(float(fv or 0))
                    B.check(L.immtsf_adam_prepare(S.g.ptr, None, n, S.scratch.ptr, S.step.ptr, S.drop.ptr,
                                                  None if pv is None else pending.ptr, None if ev is None else err.ptr,
                                                  None if hv is None else gh.ptr, None if fv is None else gf.ptr, S.skip.ptr,
                                                  B.stream_ptr()), "adam_prepare")
                    skip = int(pv == 0 or bool(ev) or bool(hv) or bool(fv))
                    what = (pv, ev, hv, fv)
                    assert int(S.skip.t[0]) == skip, what
                    assert int(pending.t[0]) == 0 and int(err.t[0]) == (ev or 0), what
                    assert int(S.step.t[0]) == 5 + (1 - skip) and int(S.drop.t[0]) == 10, what
                    assert S.intact() and all(x.intact() for x in (pending, err, gh, gf)), what
                    seen += 1
    assert seen == 144
    # every optional output NULL: only the partials are written
    S.load(init, 5, drop0=9)
    B.check(L.immtsf_adam_prepare(S.g.ptr, None, n, S.scratch.ptr, None, None, None, None, None, None, None, B.stream_ptr()), "adam_prepare")
    g64 = init[1].double()
    _check_partials(S, float((g64 * g64).sum()), n, "prepare, all NULL")
    assert int(S.step.t[0]) == 5 and int(S.drop.t[0]) == 9 and S.intact()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [40, 4099])
def test_dropped_step_changes_nothing_but_the_zero_fill(n, offset):
    dev = _dev()
    B, L = _lib()
    S = State(dev, n, offset, twin=offset)
    base = R.family_base(n, 7)
    init = [torch.from_numpy(a).to(dev) for a in R.family_case(base, 1e-3, 1.0, 3)]
    ibits = [x.view(torch.int32) for x in init]
    h = _hp(1e-3, 1.0)
    lo, hi = 8, (n - 11) | 1          # an odd hi

    def unchanged(what):
        assert S.intact(), what
        for x, w in zip((S.p, S.m, S.v), (ibits[0], ibits[2], ibits[3])):
            assert torch.equal(x.b, w), (what, "a dropped step wrote p / m / v")
        assert bool((S.twin.t == 0x1234).all()), (what, "a dropped step wrote the twin")

    B.check(L.immtsf_bf16_twin_register(S.p.ptr, S.twin.ptr, n), "twin_register")
    try:
        for zero in (0, 1):
            # adam_range behind a non-zero skip word (prepare not called: the partials are NaN and must not matter)
            S.load(init, 2)
            S.skip.t.fill_(1)
            r_range(B, L, S, h, 3, pieces=[(lo, hi)], zero=zero, prepare=False)
            unchanged(f"adam_range zero_grad={zero}")
            assert int(S.step.t[0]) == 2 and int(S.drop.t[0]) == 41
            want = ibits[1].clone()
            if zero:
                want[lo:hi] = 0
            assert torch.equal(S.g.b, want), ("adam_range: the zero-fill of a dropped step is exactly grad[lo, hi) with zero_grad, nothing otherwise", zero)
            # prepare that decides to drop (a time-out word), then the ranges
            S.load(init, 2)
            err = Guarded(dev, 1, torch.int32)
            err.t.fill_(7)
            B.check(L.immtsf_adam_prepare(S.g.ptr, None, n, S.scratch.ptr, S.step.ptr, S.drop.ptr, None, err.ptr, None, None, S.skip.ptr,
                                          B.stream_ptr()), "adam_prepare")
            r_range(B, L, S, h, 3, pieces=3, zero=zero, prepare=False)
            unchanged(f"prepare(err) + ranges zero_grad={zero}")
            assert int(S.step.t[0]) == 2 and int(S.drop.t[0]) == 42 and int(S.skip.t[0]) == 1
            assert bool((S.g.b == 0).all()) if zero else torch.equal(S.g.b, ibits[1])
            # adam_step_guarded behind a non-zero skip word
            S.load(init, 2)
            S.skip.t.fill_(3)
            r_guarded(B, L, S, h, 3, zero=zero)
            unchanged(f"adam_step_guarded zero_grad={zero}")
            assert int(S.step.t[0]) == 2 and int(S.drop.t[0]) == 42, "a dropped step is not counted; the dropout counter still advances"
            assert bool((S.g.b == 0).all()) if zero else torch.equal(S.g.b, ibits[1])
    finally:
        L.immtsf_bf16_twin_unregister(S.p.ptr)


def test_guard_pack():
    dev = _dev()
    B, L = _lib()
    err = Guarded(dev, 1, torch.int32)
    for e in (0, 5):
        err.t.fill_(e)
        for is_bf16, dtype, one in ((0, torch.float32, 0x3F800000), (1, torch.int16, 0x3F80)):
            slot = Guarded(dev, 3, dtype)
            slot.b.fill_(0x1234)
            B.check(L.immtsf_guard_pack(err.ptr, _at(slot, 1), is_bf16, B.stream_ptr()), "guard_pack")
            assert [int(x) for x in slot.b.cpu()] == [0x1234, one if e else 0, 0x1234], (e, is_bf16)
            assert slot.intact() and err.intact() and int(err.t[0]) == e


# ---- g. under replay ---------------------------------------------------------------------------------------------------------------

def test_prepare_and_ranges_under_graph_replay():
    """one single-stream capture of adam_prepare + three adam_range pieces with zero_grad, replayed three times with a fresh gradient each:
    replay k uses bias correction k (the device counter, not a value frozen at capture), leaves the gradient zero, and is one step of
    the reference from the device state before it"""
    dev = _dev()
    B, L = _lib()
    n = 4099
    wd, max_norm = 1e-3, 1.0
    S = State(dev, n, 0)
    base = R.family_base(n, 8)
    p0, g0, m0, v0 = R.family_case(base, wd, max_norm, 1)
    grads = [g0] + [R.family_case(R.family_base(n, 8 + k), wd, max_norm, 1)[1] for k in (1, 2)]
    init = [torch.from_numpy(a).to(dev) for a in (p0, g0, m0, v0)]
    h = _hp(wd, max_norm)
    side = torch.cuda.Stream()
    S.load(init, 0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r_range(B, L, S, h, 1, pieces=3, zero=1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r_range(B, L, S, h, 1, pieces=3, zero=1)
    S.load(init, 0)
    worst = {}
    for k in (1, 2, 3):
        S.g.t.copy_(torch.from_numpy(grads[k - 1]).to(dev))
        before = [x.t.cpu().numpy().copy() for x in (S.p, S.g, S.m, S.v)]
        graph.replay()
        torch.cuda.synchronize()
        ref = R.clip_adam_f64(*before, R.LR, R.B1, R.B2, R.EPS, wd, k, max_norm)
        _check_update(S, DevRef(ref, dev), f"replay {k}", worst)
        _check_partials(S, ref.norm_sq, n, f"replay {k}")
        assert bool((S.g.b == 0).all()) and S.intact()
        assert int(S.step.t[0]) == k and int(S.drop.t[0]) == 41 + k
        if k > 1:       # the yardstick resolves the step number: the previous step's bias corrections are far outside it
            stale = R.clip_adam_f64(*before, R.LR, R.B1, R.B2, R.EPS, wd, k - 1, max_norm)
            assert R.ratio_to_yardstick(stale.p, ref.p, ref.Yp) > 100 * R.K
    print("replay: worst ratio (p, m, v):", {k: [round(x, 3) for x in w] for k, w in worst.items()})
