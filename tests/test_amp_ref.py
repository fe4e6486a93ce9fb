"""CPU checks of the loss-scaled optimizer step's yardstick and host-side surface: tests/amp_ref.py against torch itself (GradScaler on
the CPU + torch.optim.Adam + clip_grad_norm_ on a float64 parameter, in main.py's order and in torch's unscale_-first order), against
the project's float64 clip + Adam reference, and what immtsf.optim promises without a GPU."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import amp_ref as A  # noqa: E402
from oracle import optimizer_ref as R  # noqa: E402

HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, max_norm=1.0)
N = 37


def _grads(step):
    """the true (unscaled) gradient of each of the six steps: given, not computed -- small enough that only the scaled norm is clipped"""
    rng = np.random.default_rng(100 + step)
    return rng.standard_normal(N) * 10.0 ** rng.uniform(-4.0, -1.0, N)


def _torch_loop(unscale_first):
    from immtsf import optim
    p = torch.nn.Parameter(torch.from_numpy(np.random.default_rng(7).standard_normal(N)))
    assert p.dtype == torch.float64
    opt = optim._torch_adam([p], lr=HP["lr"], weight_decay=HP["wd"])
    scaler = torch.amp.GradScaler("cpu", init_scale=A.PATTERN_INIT, growth_interval=A.PATTERN_INTERVAL)
    trace = []
    for i in range(6):
        opt.zero_grad()
        (scaler.scale((p * torch.from_numpy(_grads(i))).sum())).backward()       # .grad = S g
        if A.PATTERN_FOUND[i]:
            p.grad[N // 2] = float("inf")
        if unscale_first:
            scaler.unscale_(opt)
        optim._torch_clip([p], HP["max_norm"])
        scaler.step(opt)
        scaler.update()
        st = opt.state[p]
        trace.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy() if st else np.zeros(N),
                      st["exp_avg_sq"].numpy().copy() if st else np.zeros(N), int(st["step"]) if st else 0, float(scaler.get_scale()),
                      int(scaler._growth_tracker)))
    return trace


def _ref_loop(unscale_first):
    p = np.random.default_rng(7).standard_normal(N)
    m, v, step, scale, tracker, trace = np.zeros(N), np.zeros(N), 0, A.PATTERN_INIT, 0, []
    for i in range(6):
        g = np.float64(scale) * _grads(i)
        if A.PATTERN_FOUND[i]:
            g[N // 2] = np.inf
        if unscale_first:
            with np.errstate(invalid="ignore"):
                r = A.scaled_step(p, g * A.inv_scale(scale), m, v, step, scale=None, **HP)
        else:
            r = A.scaled_step(p, g, m, v, step, scale=scale, **HP)
        assert r.skip == A.PATTERN_FOUND[i]
        p, m, v, step = r.p, r.m, r.v, r.step
        scale, tracker = A.scale_update(scale, tracker, r.found_inf, interval=A.PATTERN_INTERVAL)
        trace.append((p, m, v, step, scale, tracker))
    return trace


def _compare(unscale_first):
    got, ref = _torch_loop(unscale_first), _ref_loop(unscale_first)
    for i, (t, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), t[:3], r[:3]):
            # both sides are float64 evaluations of the same formula in slightly different operation orders (torch's addcdiv, its
            # lerp for exp_avg): a few ulp of float64 per step, 1e-12 relative to the largest entry leaves three orders of room
            assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), (unscale_first, i, name)
        assert t[3:] == r[3:], (unscale_first, i, t[3:], r[3:])
    return ref


def test_restatement_matches_torch_in_main_py_order():
    ref = _compare(False)
    # the scale halves at the step with the inf, the step count stays where it was, three clean steps double the scale again
    assert [r[3] for r in ref] == [1, 2, 2, 3, 4, 5]
    assert [r[4] for r in ref] == [65536.0, 65536.0, 32768.0, 32768.0, 32768.0, 65536.0]
    assert [r[5] for r in ref] == [1, 2, 0, 1, 2, 0]
    assert [(r[4], r[5]) for r in ref] == A.pattern_scales()


def test_restatement_matches_torch_with_unscale_before_the_clip():
    _compare(True)


def test_the_two_orders_differ_visibly():
    """clipping S g and clipping g are different updates (the scaled norm is always far above max_norm, the true one here never): the
    reason the fused step must know which gradient it was handed"""
    a, b = _ref_loop(False), _ref_loop(True)
    assert np.abs(a[0][1] - b[0][1]).max() > 0.1 * np.abs(a[0][1]).max()


def test_restatement_agrees_with_the_optimizer_reference():
    """amp_ref.scaled_step and oracle/optimizer_ref.clip_adam_f64 (the yardsticks of the GPU tests) state the same update: the latter with
    the unscaled gradient g inv and the norm of the stored one"""
    rng = np.random.default_rng(3)
    n = 203
    p, m = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 1e-2).astype(np.float32)
    v, g = (rng.standard_normal(n) * 1e-2).astype(np.float32) ** 2, (rng.standard_normal(n) * 1000.0).astype(np.float32)
    hp = dict(lr=R.f32(R.LR), b1=R.f32(R.B1), b2=R.f32(R.B2), eps=R.f32(R.EPS), wd=R.f32(1e-3))
    for scale in (None, 1.0, 65536.0, 1000.0):
        for max_norm in (0.0, 1.0, 1e12):
            a = A.scaled_step(p, g, m, v, 2, max_norm=max_norm, scale=scale, clip_eps=R.f32(1e-6), **hp)
            r = R.clip_adam_f64(p.astype(np.float64), g.astype(np.float64) * A.inv_scale(scale), m, v, R.LR, R.B1, R.B2, R.EPS, 1e-3, 3,
                                max_norm, norm_sq=a.norm_sq)
            for x, y in ((a.p, r.p), (a.m, r.m), (a.v, r.v)):
                assert np.abs(x - y).max() <= 1e-13 * np.abs(y).max(), (scale, max_norm)


def test_scale_update_does_not_grow_to_inf():
    big = float(np.finfo(np.float32).max)
    assert A.scale_update(big, 2, False, interval=3) == (big, 0)
    assert A.scale_update(4.0, 0, True) == (2.0, 0)


def test_adam_still_returns_torch_adam_where_it_did():
    """nothing about the constructor's routing changed: CPU parameters, several groups, amsgrad, a tensor lr -> torch's Adam"""
    from immtsf import optim
    w = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))]
    assert type(optim.Adam(w)) is optim._torch_adam
    assert type(optim.Adam(w, amsgrad=True)) is optim._torch_adam
    assert type(optim.Adam([{"params": [w[0]]}, {"params": [w[1]], "lr": 1e-2}])) is optim._torch_adam
    assert type(optim.Adam(w, lr=torch.tensor(1e-3))) is optim._torch_adam
    assert type(optim.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], weight_decay=0.01)) is optim._torch_adam


def test_fused_adam_advertises_the_loss_scale_contract():
    """GradScaler.step() looks for `_step_supports_amp_scaling` and then for NO `grad_scaler` keyword on step() (it would pass itself)"""
    import inspect

    from immtsf import _lib, config, optim
    assert optim.FusedAdam._step_supports_amp_scaling is True
    assert "grad_scaler" not in inspect.signature(optim.FusedAdam.step).parameters
    assert isinstance(config.optim_amp, bool)
    assert {"immtsf_adam_prepare_scaled", "immtsf_adam_range_scaled", "immtsf_loss_scale_update"} <= set(_lib.exported_names())
    hdr = open(os.path.join(ROOT, "include", "immtsf.h")).read()
    assert f"#define IMMTSF_AMP_SCRATCH_FLOATS {_lib.AMP_SCRATCH_FLOATS}" in hdr
