"""float64 restatement of ONE loss-scaled clip + Adam step and of the loss-scale update, numpy only.  TEST INFRASTRUCTURE ONLY.

The loop it restates is the reference's --use_amp branch (main.py:1080-1091): `scaler.scale(loss).backward()`, `clip_grad_norm_(params,
max_norm)`, `scaler.step(optimizer)`, `scaler.update()` -- nothing unscales before the clip, so with g the gradient AS STORED (S times
the true one):

    found_inf = found_inf_in or any element of g is inf / NaN          (element by element: not read off the norm)
    skip      = found_inf                                              -> p, m, v and the step count stay as they are
    coef      = min(1, max_norm / (||g|| + clip_eps))   if max_norm > 0 else 1          torch's clip_grad_norm_, on the stored gradient
    inv       = float32(1 / S)                                                          torch's _unscale_grads_: a double reciprocal, rounded
    g'        = (g coef) inv + wd p                                                     clip, then unscale, then L2-style weight decay
    m' = b1 m + (1 - b1) g' ;  v' = b2 v + (1 - b2) g'^2 ;  t = step + 1
    p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

`scaler.unscale_(opt)` before the clip (torch's documented recipe) is the same function with the unscaled gradient and scale = None.
tests/test_amp_ref.py pins both orders, the skip and the scale update against torch itself on the CPU."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Step = namedtuple("Step", "p m v step skip found_inf coef inv norm_sq")


def inv_scale(scale):
    """the reciprocal torch multiplies by: formed in double, rounded to float32 (scale None: 1)"""
    return 1.0 if scale is None else float(np.float32(1.0 / float(scale)))


def scaled_step(p, g, m, v, step, *, lr, b1, b2, eps, wd, max_norm, scale=None, found_inf_in=False, clip_eps=1e-6):
    """p, m, v: the state (widened exactly); g: the gradient as stored; step: steps taken so far.  Returns Step (float64 arrays)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    found = bool(found_inf_in) or not bool(np.isfinite(g).all())
    inv = inv_scale(scale)
    if found:
        return Step(p, m, v, step, True, True, None, inv, None)
    norm_sq = float(np.dot(g, g))
    coef = min(1.0, max_norm / (np.sqrt(norm_sq) + clip_eps)) if max_norm > 0 else 1.0
    gp = (g * coef) * inv + wd * p
    m2 = b1 * m + (1 - b1) * gp
    v2 = b2 * v + (1 - b2) * gp * gp
    t = step + 1
    p2 = p - (lr / (1 - b1 ** t)) * m2 / (np.sqrt(v2) / np.sqrt(1 - b2 ** t) + eps)
    return Step(p2, m2, v2, t, False, False, coef, inv, norm_sq)


def scale_update(scale, tracker, found_inf, growth=2.0, backoff=0.5, interval=2000):
    """torch's _amp_update_scale_ on float32 values: -> (scale, tracker)"""
    scale = np.float32(scale)
    if found_inf:
        return float(np.float32(scale * np.float32(backoff))), 0
    ok = tracker + 1
    if ok == interval:
        with np.errstate(over="ignore"):
            grown = np.float32(scale * np.float32(growth))
        return (float(grown) if np.isfinite(grown) else float(scale)), 0
    return float(scale), ok


# the six-step pattern the CPU pin and the GPU tests share: an inf in the gradient at step 2, growth interval 3
PATTERN_FOUND = (False, False, True, False, False, False)
PATTERN_INIT, PATTERN_INTERVAL = 65536.0, 3


def pattern_scales():
    """(scale, tracker) after each of the six updates"""
    s, t, out = PATTERN_INIT, 0, []
    for f in PATTERN_FOUND:
        s, t = scale_update(s, t, f, interval=PATTERN_INTERVAL)
        out.append((s, t))
    return out
