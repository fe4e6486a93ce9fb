"""CPU checks behind tests/test_gpu_attention.py: the float64 restatement of dense attention (tests/attention_ref.py) equals the reference's
golden and torch's scaled_dot_product_attention; its live mask, packed and shared-K/V forms are the dense form; the shapes of
tests/attention_cases.py reach the kernel instances they are listed for; the "extreme logits" inputs have the properties the GPU test relies
on; the per-slice error measure sees what the whole-tensor one hides.  The restatement's backward is float64 autograd, not written out,
so there is no gradcheck.
Bars: the golden is float32 (stored values rounded to 6e-8 relative, the reference's own float32 sums over at most 7 keys x 4 columns a
few units of that): 2e-6 of the largest element.  float64 against float64: 1e-12."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as C  # noqa: E402
import attention_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64_BAR = 1e-12


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def _keep(shape, seed, p=0.3):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= p).to(torch.uint8)


def test_restatement_equals_the_reference_golden():
    z = np.load(os.path.join(GOLDEN, "layer_full_attention.npz"))
    q, k, v, up = (torch.from_numpy(z[n]) for n in ("q", "k", "v", "upstream"))
    got = R.attention_forward_backward(q, k, v, up, q.shape[-1] ** -0.5)
    for g, name in zip(got, ("out", "gq", "gk", "gv")):
        err = _rel(g, torch.from_numpy(z[name]).double())
        assert err < 2e-6, (name, err)


@pytest.mark.parametrize("shape", [(2, 7, 7, 3, 8, 8), (3, 5, 9, 2, 4, 6), (1, 1, 1, 1, 4, 4), (2, 9, 4, 1, 5, 3)])
@pytest.mark.parametrize("causal", [False, True])
def test_restatement_equals_torch_sdpa(shape, causal):
    B, L, S, H, E, D = shape
    q, k, v, up = (t.double() for t in C.dense_inputs(shape))
    scale = E ** -0.5
    got = R.attention_forward_backward(q, k, v, up, scale, causal)
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    mask = torch.ones(L, S, dtype=torch.bool).tril() if causal else None        # key s <= query l, also where L != S
    want = F.scaled_dot_product_attention(q2.transpose(1, 2), k2.transpose(1, 2), v2.transpose(1, 2), attn_mask=mask, scale=scale).transpose(1, 2)
    (want * up).sum().backward()
    for g, w in zip(got, (want.detach(), q2.grad, k2.grad, v2.grad)):
        assert (g - w).abs().max() <= F64_BAR * max(float(w.abs().max()), 1e-300)


@pytest.mark.parametrize("shape", [(2, 7, 7, 3, 8, 8), (3, 5, 9, 2, 4, 6)])
@pytest.mark.parametrize("causal", [False, True])
def test_restatement_with_dropout_equals_a_written_out_softmax(shape, causal):
    """the keep mask as a multiplicative mask on a hand-written softmax: max, exp, sum, divide"""
    B, L, S, H, E, D = shape
    p = 0.3
    q, k, v, up = (t.double() for t in C.dense_inputs(shape))
    keep = _keep((B, H, L, S), 3)
    scale = E ** -0.5
    got = R.attention_forward_backward(q, k, v, up, scale, causal, keep, p)
    q2, k2, v2 = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = torch.zeros(B, L, H, D, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            for l in range(L):      # noqa: E741
                n = min(S, l + 1) if causal else S
                s = scale * (k2[b, :n, h] @ q2[b, l, h])
                e = torch.exp(s - s.max())
                a = e / e.sum() * keep[b, h, l, :n].double() / (1.0 - p)
                out[b, l, h] = a @ v2[b, :n, h]
    (out * up).sum().backward()
    for g, w in zip(got, (out.detach(), q2.grad, k2.grad, v2.grad)):
        assert _rel(g, w) <= F64_BAR


def test_live_mask_zeroes_whole_windows_and_moves_nothing():
    shape = (3, 5, 9, 2, 4, 6)
    B, L, S, H, E, D = shape
    q, k, v, up = C.dense_inputs(shape)
    keep = _keep((B, H, L, S), 4)
    live = torch.tensor([1, 0, 1], dtype=torch.uint8)
    got = R.attention_forward_backward(q, k, v, up, 0.5, False, keep, 0.3, live)
    want = R.attention_forward_backward(q, k, v, up, 0.5, False, keep, 0.3)
    for g, w in zip(got, want):
        assert torch.equal(g[1], torch.zeros_like(g[1])) and torch.equal(g[0], w[0]) and torch.equal(g[2], w[2])
    sc = torch.randn(B, H, L, S, generator=torch.Generator().manual_seed(1))
    dA = torch.randn(B, H, L, S, generator=torch.Generator().manual_seed(2))
    P, A, dS = R.softmax_rows_forward_backward(sc, dA, True, keep, 0.3, live)
    P0, A0, dS0 = R.softmax_rows_forward_backward(sc, dA, True, keep, 0.3)
    for g, w in ((P, P0), (A, A0), (dS, dS0)):
        assert not g[1].any() and torch.equal(g[0], w[0]) and torch.equal(g[2], w[2])
    assert (P0.sum(-1) - 1).abs().max() < F64_BAR and not P0[:, :, 0, 1:].any()       # rows sum to one; causal row 0 sees key 0 only


def test_packed_and_shared_forms_are_the_dense_form():
    B, L, H, E, S = 3, 5, 2, 4, 7
    qkv, up = C.packed_inputs((B, L, H, E))
    keep = _keep((B, H, L, L), 5)
    out, dqkv = R.attention_qkv_forward_backward(qkv, up, 0.5, True, keep, 0.3)
    want = R.attention_forward_backward(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], up, 0.5, True, keep, 0.3)
    assert torch.equal(out, want[0]) and all(torch.equal(dqkv[:, :, i], want[1 + i]) for i in range(3))
    # shared K / V: window b alone is the dense form with rows b L .. b L + L - 1 of the (H, B L, S) mask; dk, dv add up over the windows
    q, k, v, up = C.shared_inputs((B, L, H, E, S))
    keep = _keep((H, B * L, S), 6)
    out, dq, dk, dv = R.shared_kv_forward_backward(q, k, v, up, 0.5, keep, 0.3)
    sk, sv = torch.zeros_like(dk), torch.zeros_like(dv)
    for b in range(B):
        kb = keep[:, b * L:(b + 1) * L].unsqueeze(0)
        o, gq, gk, gv = R.attention_forward_backward(q[b:b + 1], k[None], v[None], up[b:b + 1], 0.5, False, kb, 0.3)
        assert _rel(out[b], o[0]) <= F64_BAR and _rel(dq[b], gq[0]) <= F64_BAR
        sk += gk[0]
        sv += gv[0]
    assert _rel(dk, sk) <= F64_BAR and _rel(dv, sv) <= F64_BAR


# ---- the shapes reach what they are listed for
def test_short_shapes_reach_their_instances():
    for (B, L, H, E), fwd, bwd in C.SHORT:
        assert L <= 8 and E <= 64 and E % 4 == 0, "not routed to the short kernel"
        assert C.short_instance(L, H, E, 3) == fwd and C.short_instance(L, H, E, 4) == bwd, (B, L, H, E)
    reached = {(d, inst) for _, fwd, bwd in C.SHORT for d, inst in (("fwd", fwd), ("bwd", bwd))}
    assert reached == {(d, i) for d in ("fwd", "bwd") for i in ("staged<2,8>", "staged<4,8>", "staged<8,16>", "unstaged<8,16>")}
    assert any(f.startswith("staged") and b.startswith("unstaged") for _, f, b in C.SHORT)
    for (B, L, H, E), fwd, bwd in C.SHORT:      # a partial last workgroup somewhere in every instance
        if fwd.startswith("staged"):
            assert B % C.short_stage_seqs(L, H, E, 3) != 0
    assert any(f.startswith("unstaged") and (B * H * L) % 256 != 0 and B * H * L > 256 for (B, L, H, E), f, _ in C.SHORT)
    for B, L, H, E in C.QKV_GEMM:
        assert L > 8 or E % 4 != 0 or E > 64


def test_mid_and_gemm_shapes_reach_their_paths():
    assert all(C.mid_supported(L, S, E, D) for _, L, S, _, E, D in C.MID)
    B, L, S, H, E, D = C.MID[0]
    assert L * S == 1024 and C.mid_lds_bytes(L, S, E, D, False) == 99840 and C.mid_lds_bytes(L, S, E, D, True) == 133120
    assert all(C.mid_lds_bytes(L, S, E, D, True) <= 64 * 1024 for _, L, S, _, E, D in C.MID[1:])
    assert any(L % 4 and S % 8 == 1 and E < 256 for _, L, S, _, E, D in C.MID)
    assert any(D > E for *_, E, D in C.MID) and any(D < E for *_, E, D in C.MID)
    assert not any(C.mid_supported(L, S, E, D) for _, L, S, _, E, D in C.GEMM[:3]) and C.mid_supported(*C.GEMM[3][1:3], *C.GEMM[3][4:])
    assert any(S > 64 and E % 4 for _, L, S, _, E, D in C.GEMM)
    assert C.LIVE[3] > 64 and any(s[4] > 64 for s in C.SHARED)


# ---- the extreme-logit inputs
@pytest.mark.parametrize("B,L,S,H", [(2, 8, 8, 2), (2, 32, 32, 2), (1, 4, 3, 2)])
def test_extreme_inputs_have_their_properties(B, L, S, H):
    q, k, v, up = C.extreme_inputs(B, L, S, H)
    assert C.EXTREME_SCALE == C.EXTREME_E ** -0.5 == 0.25
    for t in (q, k):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) == 6.0
    s64 = C.EXTREME_SCALE * torch.einsum("blhe,bshe->bhls", q.double(), k.double())
    s32 = C.EXTREME_SCALE * torch.einsum("blhe,bshe->bhls", q, k)
    assert torch.equal(s32.double(), s64) and torch.equal(s64 * 4, (s64 * 4).round())       # exact in float32
    assert float(s64.abs().max()) == 144.0
    hidden = torch.ones(L, S, dtype=torch.bool).triu(1)
    for causal in (False, True):
        s = s64.masked_fill(hidden, float("-inf")) if causal else s64
        row_max = s.amax(-1)
        assert (row_max > 89).any(), "no row whose largest score overflows exp in float32"
        assert (row_max < -89).any(), "no row whose every score underflows exp in float32"
        naive = torch.exp(s.float()).sum(-1)          # the softmax denominator without the max subtraction
        assert torch.isinf(naive).any() and (naive == 0).any()
        P, _ = R.softmax_rows(s64, causal)
        assert torch.isfinite(P).all() and (P.sum(-1) - 1).abs().max() < F64_BAR
        # not every row is saturated: the gradients of the scores still carry information
        assert ((P > 1e-3) & (P < 1 - 1e-3)).any(-1).float().mean() > 0.25
    assert int((~hidden[0]).sum()) == 1       # causal row 0 sees a single key
    # a score of 144 next to scores more than 88 below: every other exp of that row falls under float32's smallest normal
    top = s64[-1, -1, 3]
    assert float(top[2]) == 144.0 and float(top[torch.arange(S) != 2].max()) < 144.0 - 88.0


# ---- the error measure
def test_slice_error_sees_a_wrong_quiet_slice():
    want = torch.randn(2, 5, 3, 4, generator=torch.Generator().manual_seed(0)).double()
    want[1, :, 2] *= 1e-3
    got = want.clone()
    got[1, 0, 2, 0] += 1e-4 * float(want[1, :, 2].abs().max())
    whole = float((got - want).abs().max() / want.abs().max())
    err, i = C.slice_error(got, want)
    assert whole < 1e-6 and 0.9e-4 < err < 1.1e-4 and i == 1 * 3 + 2
    zero = torch.zeros(2, 5, 3, 4)
    assert C.slice_error(zero, zero) == (0.0, 0)
    assert C.slice_error(zero + 1e-30, zero)[0] == float("inf")
    assert C.slice_error(want * float("nan"), want)[0] == float("inf")
    w2 = want.clone()
    w2[0, :, 1] = 0          # an all-zero slice in a live tensor: the floor of 1e-6 of the largest element
    g2 = w2.clone()
    g2[0, 0, 1, 0] = 1e-7 * float(w2.abs().max())
    assert abs(C.slice_error(g2, w2)[0] - 0.1) < 1e-9
    assert C.slice_error(want.permute(0, 2, 1, 3), want.permute(0, 2, 1, 3), dims=(0, 1))[0] == 0.0
