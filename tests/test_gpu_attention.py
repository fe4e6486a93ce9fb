"""GPU checks of the dense-attention kernels behind immtsf.ops.full_attention / full_attention_qkv / shared_kv_attention -- the short
kernels (csrc/attn.hip: attn_short_*, every staged instance and the unstaged one, both directions), csrc/attn_mid.hip, and the batched
GEMMs around immtsf_softmax_rows_* -- against the float64 restatement tests/attention_ref.py (pinned on the CPU by
tests/test_attention_ref.py, which also holds the shapes of tests/attention_cases.py to the instances they are listed for).  Every case:
the output and ALL input gradients; plain, causal (L == S), dropout 0.3 under the mask exported by ops.dropout_keep_mask, and both.

Error measure: per (batch, head) slice, max |got - want| / max |want| of that slice (floor 1e-6 of the tensor's largest element), the
worst slice reported (attention_cases.slice_error).  Bars, the project's own: the exact-fp32 kernels (short, attn_mid,
softmax_rows on its own) 1e-5 outputs / 1e-4 gradients; the fp32 batched-GEMM path 1e-4 / 2e-4; bf16 mode on the GEMM path relative L2
per tensor 3e-2 / 4e-2.  None is widened for the per-slice measure: the same formula in float32 torch on the CPU, measured per slice
against float64 on these very inputs, stays at or below 1.3e-6 on the outputs and 7.1e-6 on the gradients under seeded masks, and at
1.1e-5 on the gradients of its worst case under the kernels' own mask (the causal L = 2 sequences of (37, 2, 1, 32), where one
near-saturated two-key softmax row is all a slice's dq and dk have), so every bar is more than 4x that figure.
A slice whose gradient is exactly 0 in float64 -- every row sees one key, or has every key dropped -- has a bound of 1e-6 of the tensor's
largest element, or 0 where the whole tensor is 0: the kernels have to return it as 0, not as the rounding residue of dA x dropout
scale (common.hpp: mul_rounded).  (5, 1, 3, 4) and (37, 2, 1, 32) with dropout are such cases."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as C  # noqa: E402
import attention_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EXACT_BARS = (1e-5, 1e-4)        # outputs, gradients
GEMM_BARS = (1e-4, 2e-4)
BF16_L2_BARS = (3e-2, 4e-2)
P_DROP, SEED, SITE = 0.3, 0x5EED0A77, 21
BLHE, BHLS = (0, 2), (0, 1)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _nothing_more_after_a_device_error():
    """a launch that failed on the device leaves the process unusable: end the session rather than launch the remaining cases on it"""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error, no further case is launched: {e}", returncode=3)


def _vid(v):
    return v[0]


def _keep(n, p, shape):
    """the mask the kernels draw for (SEED, SITE), or None; its kept fraction within a binomial 5 sigma of 1 - p"""
    if p <= 0.0:
        return None
    from immtsf import ops
    keep = ops.dropout_keep_mask(SEED, SITE, n, p, _dev()).cpu()
    assert abs(float(keep.double().mean()) - (1.0 - p)) <= 5.0 * math.sqrt(p * (1.0 - p) / n), (float(keep.double().mean()), n)
    return keep.view(*shape)


def _assert_close(label, names, got, want, dims, bars):
    bad = []
    for i, (n, g, w) in enumerate(zip(names, got, want)):
        d = dims[i] if isinstance(dims, list) else dims
        bar = bars[i] if isinstance(bars, list) else bars[0] if i == 0 else bars[1]
        err, where = C.slice_error(g, w, d)
        print(f"{label} {n}: worst slice error {err:.2e} (slice {where}, bar {bar:.0e})")
        if not (torch.isfinite(torch.as_tensor(g)).all() and err < bar):
            bad.append(f"{n} {err:.2e} at slice {where} (bar {bar:.0e})")
    assert not bad, f"{label}: " + "; ".join(bad)


def _assert_close_l2(label, names, got, want, bars):
    bad = []
    for i, (n, g, w) in enumerate(zip(names, got, want)):
        bar = bars[0] if i == 0 else bars[1]
        err = C.l2_error(g, w)
        print(f"{label} {n}: relative L2 {err:.2e} (bar {bar:.0e})")
        if not (torch.isfinite(g).all() and err < bar):
            bad.append(f"{n} {err:.2e} (bar {bar:.0e})")
    assert not bad, f"{label}: " + "; ".join(bad)


# ---- runners: the public ops, forward and backward; each says which path it took
def _dense(inputs, scale, causal, p, precision="fp32"):
    """-> ((out, dq, dk, dv), took attn_mid)"""
    from immtsf import ops
    dev = _dev()
    q, k, v = (t.to(dev).requires_grad_(True) for t in inputs[:3])
    out = ops.full_attention(q, k, v, scale, p, p > 0, SEED, SITE, causal, precision)
    mid = out.grad_fn.mid
    out.backward(inputs[3].to(dev))
    return (out.detach(), q.grad, k.grad, v.grad), mid


def _packed(qkv, up, scale, causal, p, precision="fp32"):
    """-> ((out, dq, dk, dv), name of the autograd function that ran)"""
    from immtsf import ops
    dev = _dev()
    x = qkv.to(dev).requires_grad_(True)
    out = ops.full_attention_qkv(x, scale, p, p > 0, SEED, SITE, causal, precision)
    fn = type(out.grad_fn).__name__
    out.backward(up.to(dev))
    return (out.detach(), x.grad[:, :, 0], x.grad[:, :, 1], x.grad[:, :, 2]), fn


def _shared(inputs, scale, p, precision="fp32"):
    from immtsf import ops
    dev = _dev()
    q, k, v = (t.to(dev).requires_grad_(True) for t in inputs[:3])
    out = ops.shared_kv_attention(q, k, v, scale, p, p > 0, SEED, SITE, precision)
    out.backward(inputs[3].to(dev))
    return out.detach(), q.grad, k.grad, v.grad


class _gemm_path:
    """config.attn_mid switched off, restored on the way out"""

    def __enter__(self):
        from immtsf import config
        self.was = config.attn_mid
        config.attn_mid = False

    def __exit__(self, *exc):
        from immtsf import config
        config.attn_mid = self.was


# ---- float64 references: computed once per (inputs, variant), shared by the fp32 and bf16 cases
@functools.lru_cache(maxsize=None)
def _dense_reference(shape, causal, p):
    B, L, S, H, E, D = shape
    q, k, v, up = C.dense_inputs(shape)
    return R.attention_forward_backward(q, k, v, up, E ** -0.5, causal, _keep(B * H * L * S, p, (B, H, L, S)), p)


@functools.lru_cache(maxsize=None)
def _packed_reference(shape, causal, p):
    B, L, H, E = shape
    qkv, up = C.packed_inputs(shape)
    out, dqkv = R.attention_qkv_forward_backward(qkv, up, E ** -0.5, causal, _keep(B * H * L * L, p, (B, H, L, L)), p)
    return out, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]


@functools.lru_cache(maxsize=None)
def _extreme_reference(B, L, H, causal, p):
    q, k, v, up = C.extreme_inputs(B, L, L, H)
    return R.attention_forward_backward(q, k, v, up, C.EXTREME_SCALE, causal, _keep(B * H * L * L, p, (B, H, L, L)), p)


NAMES = ("out", "dq", "dk", "dv")


# ---- the short kernels
@pytest.mark.parametrize("variant", C.VARIANTS, ids=_vid)
@pytest.mark.parametrize("case", C.SHORT, ids=lambda c: "x".join(map(str, c[0])) + "_" + "_".join(c[1:]).translate({60: None, 62: None, 44: "x"}))
def test_short_kernels_against_float64(case, variant):
    """full_attention_qkv at L <= 8, E <= 64, E % 4 == 0; the instance each direction reaches is the second and third entry of the case
    (forward, backward): staged <2,8>, <4,8>, <8,16> with a partial last group, staged forward with unstaged backward, and unstaged"""
    shape, _, _ = case
    _, causal, p = variant
    qkv, up = C.packed_inputs(shape)
    got, fn = _packed(qkv, up, shape[3] ** -0.5, causal, p)
    assert fn == "ShortAttentionQKVFnBackward", fn
    _assert_close(f"short {shape} {variant[0]}", NAMES, got, _packed_reference(shape, causal, p), BLHE, EXACT_BARS)


# ---- attn_mid
@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.MID for v in C.variants(s[1], s[2])],
                         ids=lambda x: x[0] if isinstance(x[0], str) else "x".join(map(str, x)))
def test_attn_mid_against_float64(shape, variant):
    """full_attention with config.attn_mid at (B, L, S, H, E, D): the dynamic LDS above 64 KB in both directions with L S = 1024 (the
    fourth dS slot of the backward); L % 4 != 0, S % 8 = 1 and idle lanes; the narrowest heads; D << E and D >> E; one element"""
    from immtsf import _lib
    _, causal, p = variant
    assert _lib.load().immtsf_attn_mid_supported(*shape[1:3], *shape[4:]) == 1
    got, mid = _dense(C.dense_inputs(shape), shape[4] ** -0.5, causal, p)
    assert mid is True
    _assert_close(f"attn_mid {shape} {variant[0]}", NAMES, got, _dense_reference(shape, causal, p), BLHE, EXACT_BARS)


# ---- batched GEMMs + softmax_rows
@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.GEMM for v in C.variants(s[1], s[2])],
                         ids=lambda x: x[0] if isinstance(x[0], str) else "x".join(map(str, x)))
def test_gemm_path_fp32_against_float64(shape, variant):
    """full_attention where attn_mid does not apply: L, S > 32 (causal included); S > 64 -- the per-lane loop of softmax_rows runs more
    than once -- with E % 4 != 0; one element; and a shape attn_mid takes, with the knob off"""
    from immtsf import _lib
    _, causal, p = variant
    with _gemm_path():
        got, mid = _dense(C.dense_inputs(shape), shape[4] ** -0.5, causal, p)
    assert mid is False
    if shape in C.GEMM[:3]:
        assert _lib.load().immtsf_attn_mid_supported(*shape[1:3], *shape[4:]) == 0
        again, mid = _dense(C.dense_inputs(shape), shape[4] ** -0.5, causal, p)        # the knob on changes nothing for a refused shape
        assert mid is False and all(torch.equal(a, b) for a, b in zip(got, again))
    _assert_close(f"gemm fp32 {shape} {variant[0]}", NAMES, got, _dense_reference(shape, causal, p), BLHE, GEMM_BARS)


@pytest.mark.parametrize("shape,variant", [(s, v) for s in C.GEMM_BF16 for v in C.variants(s[1], s[2])],
                         ids=lambda x: x[0] if isinstance(x[0], str) else "x".join(map(str, x)))
def test_gemm_path_bf16_against_float64(shape, variant):
    _, causal, p = variant
    got, mid = _dense(C.dense_inputs(shape), shape[4] ** -0.5, causal, p, "bf16")
    assert mid is False
    _assert_close_l2(f"gemm bf16 {shape} {variant[0]}", NAMES, got, _dense_reference(shape, causal, p), BF16_L2_BARS)


@pytest.mark.parametrize("variant", C.VARIANTS, ids=_vid)
@pytest.mark.parametrize("shape", C.QKV_GEMM, ids=lambda s: "x".join(map(str, s)))
def test_packed_gemm_path_against_float64(shape, variant):
    """FullAttentionQKVFn (strided reads of the packed tensor, packed gradient): L > 8, and L = 2 with E % 4 != 0"""
    _, causal, p = variant
    qkv, up = C.packed_inputs(shape)
    got, fn = _packed(qkv, up, shape[3] ** -0.5, causal, p)
    assert fn == "FullAttentionQKVFnBackward", fn
    _assert_close(f"packed gemm {shape} {variant[0]}", NAMES, got, _packed_reference(shape, causal, p), BLHE, GEMM_BARS)


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["plain", "dropout"])
@pytest.mark.parametrize("shape", C.SHARED, ids=lambda s: "x".join(map(str, s)))
def test_shared_kv_against_float64(shape, p):
    """SharedKVAttentionFn at (B, L, H, E, S): S > 64, and one query with one key; the scores and the mask live as (H, B L, S)"""
    B, L, H, E, S = shape
    inputs = C.shared_inputs(shape)
    got = _shared(inputs, E ** -0.5, p)
    want = R.shared_kv_forward_backward(*inputs, E ** -0.5, _keep(H * B * L * S, p, (H, B * L, S)), p)
    _assert_close(f"shared kv {shape} p={p}", NAMES, got, want, [BLHE, BLHE, (1,), (1,)], GEMM_BARS)


# ---- the live mask of the row softmax, through the C ABI
@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["plain", "dropout"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_softmax_rows_live_mask(causal, p):
    """immtsf_softmax_rows_forward / _backward with live = [1, 0, 1]: the dead window is exactly 0 in P, A and dS; the live windows match
    float64 with the dropout mask at their own indices, and are bit for bit what a call without the mask gives (nothing is shifted)"""
    from immtsf import _lib
    from immtsf._lib import check, ptr, stream_ptr
    dev = _dev()
    lib = _lib.load()
    B, H, L, S = C.LIVE
    g = torch.Generator().manual_seed(31)
    scores, dA = 2.0 * torch.randn(B, H, L, S, generator=g), torch.randn(B, H, L, S, generator=g)
    live = torch.tensor([1, 0, 1], dtype=torch.uint8)

    def rows(live_dev):
        P, A, G = scores.to(dev), torch.empty(B, H, L, S, device=dev), dA.to(dev)
        check(lib.immtsf_softmax_rows_forward(ptr(P), ptr(A), B, H, L, S, ptr(live_dev), p, SEED, SITE, 1 if causal else 0, None, stream_ptr()),
              "softmax_rows_forward")
        check(lib.immtsf_softmax_rows_backward(ptr(G), ptr(P), B, H, L, S, p, SEED, SITE, None, stream_ptr()), "softmax_rows_backward")
        torch.cuda.synchronize()
        return P.cpu(), A.cpu(), G.cpu()

    got = rows(live.to(dev))
    want = R.softmax_rows_forward_backward(scores, dA, causal, _keep(B * H * L * S, p, (B, H, L, S)), p, live)
    for n, t in zip(("P", "A", "dS"), got):
        assert not t[1].any(), f"{n} of the dead window is not exactly 0"
    _assert_close(f"softmax_rows live causal={causal} p={p}", ("P", "A", "dS"), got, want, BHLS, [EXACT_BARS[0], EXACT_BARS[0], EXACT_BARS[1]])
    for n, a, b in zip(("P", "A", "dS"), got, rows(None)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), f"{n}: a live window differs from the call without a live mask"


# ---- extreme logits on each of the three paths
@pytest.mark.parametrize("variant", C.VARIANTS, ids=_vid)
@pytest.mark.parametrize("path", ["short", "mid", "gemm"])
def test_extreme_logits(path, variant):
    """integer q, k in [-6, 6] at E = 16 (scale 0.25): every score is exact in float32, up to +-144; rows whose largest score is above 89,
    rows whose every score is below -89, a 144 next to scores that underflow after the subtraction, causal rows of one key (all asserted
    on the CPU in test_attention_ref.py).  What is left is expf: the ordinary bars, and everything finite"""
    _, causal, p = variant
    B, H = 2, 2
    L = 8 if path == "short" else 32
    q, k, v, up = C.extreme_inputs(B, L, L, H)
    if path == "short":
        got, fn = _packed(torch.stack([q, k, v], dim=2).contiguous(), up, C.EXTREME_SCALE, causal, p)
        assert fn == "ShortAttentionQKVFnBackward", fn
    elif path == "mid":
        got, mid = _dense((q, k, v, up), C.EXTREME_SCALE, causal, p)
        assert mid is True
    else:
        with _gemm_path():
            got, mid = _dense((q, k, v, up), C.EXTREME_SCALE, causal, p)
        assert mid is False
    assert all(torch.isfinite(t).all() for t in got)
    _assert_close(f"extreme logits {path} {variant[0]}", NAMES, got, _extreme_reference(B, L, H, causal, p), BLHE,
                  GEMM_BARS if path == "gemm" else EXACT_BARS)


# ---- determinism
@pytest.mark.parametrize("path", ["short_staged", "short_unstaged", "mid", "mid_lds_opt_in", "gemm_fp32", "gemm_bf16", "packed_gemm", "shared_kv"])
def test_two_runs_with_dropout_give_the_same_bits(path):
    def once():
        if path == "short_staged":
            return _packed(*C.packed_inputs((19, 3, 2, 20)), 20 ** -0.5, True, P_DROP)[0]
        if path == "short_unstaged":
            return _packed(*C.packed_inputs((5, 8, 9, 8)), 8 ** -0.5, True, P_DROP)[0]
        if path == "mid":
            return _dense(C.dense_inputs((2, 5, 9, 3, 252, 8)), 252 ** -0.5, False, P_DROP)[0]
        if path == "mid_lds_opt_in":
            return _dense(C.dense_inputs((1, 32, 32, 1, 256, 256)), 1 / 16, True, P_DROP)[0]
        if path in ("gemm_fp32", "gemm_bf16"):
            return _dense(C.dense_inputs((2, 37, 37, 2, 24, 24)), 24 ** -0.5, True, P_DROP, path[5:])[0]
        if path == "packed_gemm":
            return _packed(*C.packed_inputs((5, 19, 3, 8)), 8 ** -0.5, True, P_DROP)[0]
        return _shared(C.shared_inputs((3, 5, 2, 12, 70)), 12 ** -0.5, P_DROP)
    a, b = once(), once()
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), f"{path}: {n} differs between two runs"
