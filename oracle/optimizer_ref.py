"""float64 reference of the fused clip + Adam update (csrc/tail.hip adam_kernel and the norm kernels in front of it) and bit-level
references of the two bf16 streams.  TEST INFRASTRUCTURE ONLY, numpy only.

The operation (main.py:1098-1101: clip_grad_norm_(max_norm), then torch.optim.Adam with L2-style weight decay), per element:

    coef = min(1, max_norm / (||g|| + 1e-6))   if max_norm > 0 else 1
    g'   = coef g + wd p
    m'   = b1 m + (1 - b1) g'
    v'   = b2 v + (1 - b2) g'^2
    p'   = p - u,   u = (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

Hyperparameters.  The C ABI takes `float` arguments, so every hyperparameter is rounded to fp32 FIRST and then widened: the function
under test is the one with those fp32 values (a Python-double 0.999 differs from float(0.999f) by 1.3e-5 of 1 - b2, which would
otherwise be booked as kernel error).  1 - b1 and 1 - b2 are exact in fp32 (Sterbenz), the constant 1e-6 is the fp32 one.

Yardsticks.  Beside every value the reference returns the first-order propagation of ONE fp32 rounding (relative 2^-24) per
operation, evaluated in float64; a comparison passes when |got - ref| <= K 2^-24 Y for EVERY element (ratio_to_yardstick):

    Y_g = |coef g| (1 + c_n) + |wd p|
    Y_m = |b1 m| + (1 - b1) Y_g
    Y_v = b2 v + 2 (1 - b2) |g'| Y_g + (1 - b2) g'^2
    Y_p = |p| + |u| (1 + 1/(1 - b1^t) + 1/2 / (1 - b2^t)) + |du/dm| Y_m + |du/dv| Y_v

Y_g is condition-aware on purpose: coef g + wd p cancels for small g, so the error of g' (and of everything after it) is measured
against the terms, not against the result.  The two bias-correction terms of Y_p are the cancellation in 1 - b^t evaluated in fp32
(powf): its relative error is about 2^-24 / (1 - b^t), 3e-5 on 1 - b2^2, and the square root halves it.  The kernel forms these in
fp32, torch in Python doubles; that is inherent to the formulation (3e-6 of one update at worst), so the yardstick carries it.

c_n: rounding depth of the clip coefficient, in units of one rounding.  All terms of the sum of squares are positive, so every
rounding on the way is relative to the sum and the bound is relative.  Reading sqnorm_partial_kernel / adam_prepare_kernel, block_sum
(common.hpp) and the head of adam_kernel:

    one thread's fma chain     1024 x 256 threads stride over the buffer: at most ceil(n / 262144) + 8 terms, one rounding each (the
                               square is exact inside the fma; + 8: a whole float4 / bf16x8 per vector trip, and the scalar tail)
    wave_sum                   6 xor-shuffle levels                                      6
    block_sum over 4 waves     r = 0 + red[0] is exact                                   3
    sharded form               the all-reduce adds the partials of the ranks             1   (counted always: a bound)
    adam_kernel head           4 partials per thread (3), wave_sum (6), 4 waves (3)     12
                                                                          norm_depth(n) = ceil(n / 262144) + 30
    partials_depth(n) = ceil(n / 262144) + 17 is the part in front of the 1024 partials (tests compare their float64 sum with ||g||^2).

sqrtf halves the relative error of the sum and adds one rounding, `total + 1e-6f` and the division add one each:
c_n = norm_depth(n) / 2 + 3.  It applies where the clip can be active (max_norm > 0 and max_norm / (||g|| + 1e-6) < 1 + 2^-16);
fminf(1, .) is exact otherwise and c_n = 0.

K.  The stick is emulate_f32: the same formula in numpy float32, one operation at a time (no fma; numpy's pairwise sum for the norm,
so an order the kernel does not use).  Over the input family (family(), every member) its largest ratios to the yardsticks, in units of 2^-24 Y, are
    n = 4099       p 0.992    m 2.641    v 1.871
    n = 65539      p 1.055    m 3.117    v 1.933
    n = 1000003    p 1.076    m 3.233    v 2.098
(m and v peak with weight decay on -- g' then carries three roundings --, without it both stay below 2; p sits at 1 at every step,
step 2 included: the 1 - b^t terms of Y_p carry the cancellation; the maxima creep up with n as extreme values do).
K = 4 x the largest, and at least 4: 4 x 3.233 = 12.93, K = 13.  tests/test_optimizer_oracle.py re-measures the first two lengths
and asserts K / 4.  The factor 4 is for what the emulation does not do: fma contraction, another operation
order, and device powf / sqrtf / division being a few ulp instead of correctly rounded.  K is never set from what the HIP kernel gives.

Scope.  Denormal behaviour is out of scope: the input family keeps every non-zero intermediate of the reference at or above 2^-116
(family_case raises the smallest gradients where an active clip would push (1 - b2) g'^2 below that; AdamRef.min_nonzero reports it
with track_min and the CPU suite asserts it), so no fp32 operation of the kernel underflows.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

K = 13.0
U32 = 2.0 ** -24
MIN_INTERMEDIATE = 2.0 ** -116
NORM_THREADS = 1024 * 256

AdamRef = namedtuple("AdamRef", "p m v coef norm_sq Yp Ym Yv c_n min_nonzero")

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
FAMILY_WD = (0.0, 1e-3)
FAMILY_MAX_NORM = (0.0, 1.0, 1e9)
FAMILY_STEPS = (1, 2, 3, 10, 1000, 100000)


def f32(x):
    """a hyperparameter as the `float` argument the ABI receives, widened"""
    return float(np.float32(x))


def norm_depth(n):
    return -(-int(n) // NORM_THREADS) + 30


def partials_depth(n):
    return -(-int(n) // NORM_THREADS) + 17


def _min_nz(cur, *arrays):
    for a in arrays:
        a = np.abs(a)
        a = a[a != 0]
        if a.size:
            cur = min(cur, float(a.min()))
    return cur


def clip_adam_f64(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, norm_sq=None, n_norm=None, track_min=False):
    """p, g, m, v: fp32 arrays, widened exactly (float64 arrays pass through: the CPU suite carries three steps of state against
    torch's float64 Adam).  norm_sq: the global sum of squares when g is one shard of the gradient; n_norm: the length the norm
    was taken over (default g.size), for c_n.  track_min: also report the smallest non-zero intermediate (costs as much as the
    update itself).  Returns AdamRef (float64 arrays)."""
    for a in (p, g, m, v):
        assert a.dtype in (np.float32, np.float64)
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, max_norm = (f32(x) for x in (lr, b1, b2, eps, wd, max_norm))
    own_sq = float(np.dot(g, g))
    if norm_sq is None:
        norm_sq = own_sq
    norm = float(np.sqrt(norm_sq))
    coef, c_n = 1.0, 0.0
    if max_norm > 0:
        q = max_norm / (norm + f32(1e-6))
        coef = min(1.0, q)
        if q < 1.0 + 2.0 ** -16:
            c_n = norm_depth(g.size if n_norm is None else n_norm) / 2 + 3
    lo = [np.inf]

    def seen(*arrays):
        if track_min:
            lo[0] = _min_nz(lo[0], *arrays)

    cg = coef * g
    wp = wd * p
    gp = cg + wp
    seen(cg, wp, gp)
    Yg = np.abs(cg)
    Yg *= 1 + c_n
    Yg += np.abs(wp)
    del cg, wp
    b1m, g1 = b1 * m, (1 - b1) * gp
    m2 = b1m + g1
    seen(b1m, g1, m2)
    Ym = np.abs(b1m, out=b1m)
    Ym += (1 - b1) * Yg
    del g1
    b2v, g2 = b2 * v, (1 - b2) * gp * gp
    v2 = b2v + g2
    seen(b2v, g2, v2)
    np.abs(gp, out=gp)
    gp *= Yg
    gp *= 2 * (1 - b2)
    Yv = b2v
    Yv += gp
    Yv += g2
    del g2, gp, Yg
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    s = np.sqrt(v2)
    s /= np.sqrt(bc2)
    den = s + eps
    u = (lr / bc1) * m2
    u /= den
    p2 = p - u
    seen(s, u, p2)
    au = np.abs(u, out=u)
    Yp = np.abs(p, out=p)
    Yp += au * (1 + 1 / bc1 + 0.5 / bc2)
    Yp += (lr / bc1) / den * Ym
    # |du/dv| Y_v = |u| / den * (1 / (2 sqrt(v') sqrt(bc2))) Y_v = |u| (s / den) Y_v / (2 v'), and nothing where v' = 0 (then Y_v = 0)
    au *= s
    au /= den
    au *= Yv
    np.divide(au, 2 * v2, out=au, where=v2 > 0)
    au[v2 == 0] = 0.0
    Yp += au
    return AdamRef(p2, m2, v2, coef, own_sq, Yp, Ym, Yv, c_n, lo[0])


def emulate_f32(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm):
    """the same update in numpy float32, one rounding per operation: the stick K is measured with.  Returns p', m', v' (fp32)."""
    F = np.float32
    lr, b1, b2, eps, wd, max_norm = (F(x) for x in (lr, b1, b2, eps, wd, max_norm))
    one = F(1)
    coef = one
    if max_norm > 0:
        total = np.sqrt(np.sum(g * g, dtype=F))
        coef = min(one, max_norm / (total + F(1e-6)))
    gp = coef * g
    if wd != 0:
        gp = wd * p + gp
    m2 = b1 * m + (one - b1) * gp
    v2 = b2 * v + ((one - b2) * gp) * gp
    bc1 = one - np.power(b1, F(step))
    bc2s = np.sqrt(one - np.power(b2, F(step)))
    p2 = p - (lr / bc1) * m2 / (np.sqrt(v2) / bc2s + eps)
    for a in (m2, v2, p2):
        assert a.dtype == F
    return p2, m2, v2


def ratio_to_yardstick(got, ref, Y):
    """max over ALL elements of |got - ref| / (2^-24 Y); an element whose yardstick is zero must be exact (else inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(Y > 0, err / (U32 * Y), np.where(err == 0, 0.0, np.inf))
    return float(np.nanmax(r)) if not np.isnan(r).any() else float("inf")


# ---- the input family ---------------------------------------------------------------------------------------------------------

def family():
    """(wd, max_norm, step) of every member; lr, betas and eps are LR, B1, B2, EPS (eps = 1e-8, what main.py trains with)"""
    return [(wd, mn, t) for wd in FAMILY_WD for mn in FAMILY_MAX_NORM for t in FAMILY_STEPS]


def family_base(n, seed):
    """one seeded draw per (n, seed), shared by all members: gradient magnitudes log-uniform in 1e-12 .. 1e3 times a normal (|z| >= 2^-4:
    the product stays inside the stated range's spirit and away from underflow), 5 % exact zeros; p ~ N(0, 1); m, v at the gradient's
    scale (an independent normal each, on the same magnitudes)"""
    rng = np.random.default_rng([int(n), int(seed)])

    def z():
        x = rng.standard_normal(n)
        return np.copysign(np.maximum(np.abs(x), 2.0 ** -4), x)

    mag = 10.0 ** rng.uniform(-12.0, 3.0, n)
    g = mag * z()
    g[rng.random(n) < 0.05] = 0.0
    p = rng.standard_normal(n)
    m = mag * z()
    v = (mag * z()) ** 2
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def family_case(base, wd, max_norm, step):
    """the member's fp32 (p, g, m, v): m = v = 0 at step 1; where the clip is active the non-zero gradients are raised to at least
    2^-52 / coef, so that (1 - b2) (coef g)^2 >= 2^-116 (they are ~1e-13 of the norm: coef does not move)"""
    p, g, m, v = base
    if step == 1:
        m, v = np.zeros_like(m), np.zeros_like(v)
    if max_norm > 0:
        norm = float(np.sqrt(np.dot(g.astype(np.float64), g.astype(np.float64))))
        coef = min(1.0, f32(max_norm) / (norm + f32(1e-6)))
        floor = np.float32(2.0 ** -52 / coef)
        small = (g != 0) & (np.abs(g) < floor)
        if small.any():
            g = np.where(small, np.copysign(floor, g), g).astype(np.float32)
    return p, g, m, v


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------

def bf16_rne(x):
    """fp32 array -> uint16 bf16 patterns, round to nearest even on the bit pattern (+0x7FFF + lsb); NaN stays NaN (quiet bit set)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    r = ((b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((b >> np.uint32(16)) | np.uint32(0x0040)).astype(np.uint16), r)


def bf16_widen(h):
    """uint16 bf16 patterns -> fp32 (exact)"""
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


BF16_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def bf16_sweep():
    """fp32 patterns: all 65536 high halves x the low halves that decide the rounding (ties in both parities, just below / above a
    tie, carry into the exponent, overflow to inf, +-0, inf, NaN)"""
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    return np.concatenate([hi | np.uint32(lo) for lo in BF16_LOW_HALVES]).view(np.float32)
