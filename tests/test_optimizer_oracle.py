"""CPU suite that pins oracle/optimizer_ref.py, the reference tests/test_gpu_optimizer.py holds the clip + Adam kernels and the bf16
streams against: the float64 restatement against torch's own Adam + clip_grad_norm_ on float64 tensors, the bf16 bit references against
torch's conversions, and the constant K against the float32 emulation it was measured with (never against a kernel)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import optimizer_ref as R  # noqa: E402

FAMILY_LENGTHS = (4099, 65539)


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("max_norm", [1.0, 1e9, 0.0], ids=["clip_active", "clip_inactive", "clip_off"])
def test_reference_is_torch_adam_with_clip(max_norm, wd):
    n = 1000
    rng = np.random.default_rng(7)
    lr, b1, b2, eps, wd = (R.f32(x) for x in (R.LR, R.B1, R.B2, R.EPS, wd))     # both sides get the fp32-rounded hyperparameters
    pr = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    mr, vr = np.zeros(n), np.zeros(n)
    tp = torch.nn.Parameter(torch.from_numpy(pr.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    worst = 0.0
    for step in (1, 2, 3):
        g = (3.0 * rng.standard_normal(n)).astype(np.float32)
        tp.grad = torch.from_numpy(g.astype(np.float64))
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([tp], R.f32(max_norm))
            assert (float(total) > max_norm) == (max_norm == 1.0)      # "active" really clips, "inactive" really does not
        opt.step()
        ref = R.clip_adam_f64(pr, g, mr, vr, lr, b1, b2, eps, wd, step, max_norm)
        upd = np.abs(ref.p - pr)
        worst = max(worst, float(np.max(np.abs(tp.detach().numpy() - ref.p) / (np.abs(ref.p) + upd))))
        st = opt.state[tp]
        for got, want, Y in ((st["exp_avg"], ref.m, ref.Ym), (st["exp_avg_sq"], ref.v, ref.Yv)):     # (m' may cancel: its terms are the scale)
            assert np.all(np.abs(got.numpy() - want) <= 1e-13 * Y)
        pr, mr, vr = ref.p, ref.m, ref.v
    print(f"max_norm={max_norm} wd={wd}: worst |torch - ref| / (|p| + |update|) = {worst:.2e}")
    assert worst < 1e-13


def test_sharded_norm_argument():
    """a shard given the global sum of squares computes what the whole buffer computes on that shard"""
    base = R.family_base(1027, 3)
    p, g, m, v = R.family_case(base, 1e-3, 1.0, 10)
    hp = (R.LR, R.B1, R.B2, R.EPS, 1e-3, 10, 1.0)
    whole = R.clip_adam_f64(p, g, m, v, *hp)
    s = 520
    a = R.clip_adam_f64(p[:s], g[:s], m[:s], v[:s], *hp, norm_sq=whole.norm_sq, n_norm=1027)
    b = R.clip_adam_f64(p[s:], g[s:], m[s:], v[s:], *hp, norm_sq=whole.norm_sq, n_norm=1027)
    assert abs(a.norm_sq + b.norm_sq - whole.norm_sq) <= 1e-15 * whole.norm_sq
    assert a.coef == whole.coef and np.array_equal(np.concatenate([a.p, b.p]), whole.p)
    assert np.array_equal(np.concatenate([a.Yp, b.Yp]), whole.Yp)


def test_bf16_references_are_torch_bit_for_bit():
    x = R.bf16_sweep()
    assert x.size == 65536 * 6
    want = torch.from_numpy(x).to(torch.bfloat16)
    got = R.bf16_rne(x)
    wbits = want.view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert nan.sum() == 2 * (127 * 6 + 5)      # per sign: 127 NaN high halves x 6 lows, and 0x7F80 with a non-zero low half
    assert np.array_equal(got[~nan], wbits[~nan])
    assert np.array_equal(np.isnan(R.bf16_widen(got)), nan) and torch.isnan(want.float()).numpy()[nan].all()
    # ties: 0x3F808000 sits between 0x3F80 (even) and 0x3F81 -> down; 0x3F818000 -> up to 0x3F82; 0x7F7F8000 overflows to inf
    t = np.array([0x3F808000, 0x3F818000, 0x7F7F8000, 0xFF7FFFFF, 0x00008000, 0x80000001], dtype=np.uint32).view(np.float32)
    assert list(R.bf16_rne(t)) == [0x3F80, 0x3F82, 0x7F80, 0xFF80, 0x0000, 0x8000]
    h = np.arange(65536, dtype=np.uint16)
    wide = torch.from_numpy(h.view(np.int16)).view(torch.bfloat16).float().numpy()
    assert np.array_equal(R.bf16_widen(h).view(np.uint32), wide.view(np.uint32))


@pytest.mark.parametrize("n", FAMILY_LENGTHS)
def test_K_comes_from_the_float32_emulation(n):
    """emulate_f32 stays within K / 4 of the reference on every member of the family, and the family keeps its own condition: no
    non-zero intermediate of the reference below 2^-116 (denormal behaviour is out of scope)"""
    base = R.family_base(n, 0)
    worst = {"p": (0.0, None), "m": (0.0, None), "v": (0.0, None)}
    for wd, max_norm, step in R.family():
        p, g, m, v = R.family_case(base, wd, max_norm, step)
        assert abs(np.mean(g == 0) - 0.05) < 0.02 and (step > 1 or not (m.any() or v.any()))
        ref = R.clip_adam_f64(p, g, m, v, R.LR, R.B1, R.B2, R.EPS, wd, step, max_norm, track_min=True)
        assert ref.min_nonzero >= R.MIN_INTERMEDIATE, (wd, max_norm, step, ref.min_nonzero)
        assert (ref.coef < 1.0) == (max_norm == 1.0)
        ep, em, ev = R.emulate_f32(p, g, m, v, R.LR, R.B1, R.B2, R.EPS, wd, step, max_norm)
        for k, got, want, Y in (("p", ep, ref.p, ref.Yp), ("m", em, ref.m, ref.Ym), ("v", ev, ref.v, ref.Yv)):
            r = R.ratio_to_yardstick(got, want, Y)
            if r > worst[k][0]:
                worst[k] = (r, (wd, max_norm, step))
            assert r <= R.K / 4, (k, wd, max_norm, step, r)
    print(f"n={n}: worst emulation ratio to the yardstick (units of 2^-24 Y) and its member (wd, max_norm, step):", worst)
    assert R.K >= 4


def test_yardstick_catches_formula_slips():
    """the reference with one formula slip is far outside K yardsticks of itself: the bound is not slack enough to hide any of them"""
    base = R.family_base(4099, 1)
    p, g, m, v = R.family_case(base, 1e-3, 1.0, 3)
    ref = R.clip_adam_f64(p, g, m, v, R.LR, R.B1, R.B2, R.EPS, 1e-3, 3, 1.0)
    p64, g64, m64, v64 = (a.astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd = (R.f32(x) for x in (R.LR, R.B1, R.B2, R.EPS, 1e-3))
    gp = ref.coef * g64 + wd * p64
    bc1, bc2 = 1 - b1 ** 3, 1 - b2 ** 3
    slips = {
        "eps inside the root": p64 - lr / bc1 * ref.m / np.sqrt(ref.v / bc2 + eps),
        "no bc2": p64 - lr / bc1 * ref.m / (np.sqrt(ref.v) + eps),
        "no bc1": p64 - lr * ref.m / (np.sqrt(ref.v / bc2) + eps),
    }
    for what, bad in slips.items():
        assert R.ratio_to_yardstick(bad, ref.p, ref.Yp) > 100 * R.K, what
    bad_m = b1 * m64 + (1 - b1) * (ref.coef * (g64 + wd * p64))
    assert R.ratio_to_yardstick(bad_m, ref.m, ref.Ym) > 100 * R.K
    assert R.ratio_to_yardstick(b1 * m64 + (1 - b1) * gp, ref.m, ref.Ym) < 1e-6
