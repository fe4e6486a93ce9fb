"""Plain-torch float64 restatement of dense attention as layers/SelfAttention_Family.py's FullAttention computes it (scores = scale Q K^T,
TriangularCausalMask, softmax over the keys, dropout on the probabilities, mix with V), with the keep mask as an argument and the
gradients of every input through float64 autograd.  tests/test_attention_ref.py pins it to the reference's golden and to torch's
scaled_dot_product_attention on the CPU; tests/test_gpu_attention.py compares immtsf.ops.full_attention / full_attention_qkv /
shared_kv_attention and the row-softmax entry points with it.  Imports nothing of immtsf and draws nothing.

    S = scale Q K^T                (causal: key s > query l masked out)
    P = softmax_s(S) * live[b]     (live: 0 / 1 per window; a dead window has P = 0, hence a zero output and zero gradients)
    A = P * keep / (1 - p)         (keep: 0 / 1 flags, (B, H, L, S); None or p = 0: A = P)
    O = A V

Layouts: q (B, L, H, E), k (B, S, H, E), v (B, S, H, D) -> O (B, L, H, D); P, A, keep (B, H, L, S) -- element ((b H + h) L + l) S + s
of the flat mask, which is the index the kernels feed their generator."""
import torch


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def softmax_rows(scores, causal=False, keep=None, p=0.0, live=None):
    """scores (B, H, L, S), already scaled -> (P, A): what immtsf_softmax_rows_forward leaves in its two buffers"""
    B, H, L, S = scores.shape
    if causal:
        hidden = torch.ones(L, S, dtype=torch.bool).triu(1)
        scores = scores.masked_fill(hidden, float("-inf"))
    P = torch.softmax(scores, dim=-1)
    if live is not None:
        P = P * _f64(live).view(B, 1, 1, 1)
    A = P if keep is None or p <= 0.0 else P * _f64(keep).reshape(B, H, L, S) / (1.0 - p)
    return P, A


def softmax_rows_forward_backward(scores, dA, causal=False, keep=None, p=0.0, live=None):
    """-> (P, A, dS) for the loss sum(A * dA): dS is what immtsf_softmax_rows_backward leaves in place of dA (the gradient of the
    SCALED scores)"""
    s = _f64(scores).clone().requires_grad_(True)
    P, A = softmax_rows(s, causal, keep, p, live)
    (A * _f64(dA)).sum().backward()
    return P.detach(), A.detach(), s.grad.detach()


def attention(q, k, v, scale, causal=False, keep=None, p=0.0, live=None):
    """differentiable float64 forward -> (O (B, L, H, D), P (B, H, L, S))"""
    scores = scale * torch.einsum("blhe,bshe->bhls", q, k)
    P, A = softmax_rows(scores, causal, keep, p, live)
    return torch.einsum("bhls,bshd->blhd", A, v), P


def attention_forward_backward(q, k, v, upstream, scale, causal=False, keep=None, p=0.0, live=None):
    """-> (O, dq, dk, dv) for the loss sum(O * upstream)"""
    q, k, v = (_f64(t).clone().requires_grad_(True) for t in (q, k, v))
    out, _ = attention(q, k, v, scale, causal, keep, p, live)
    (out * _f64(upstream)).sum().backward()
    return out.detach(), q.grad.detach(), k.grad.detach(), v.grad.detach()


def attention_qkv_forward_backward(qkv, upstream, scale, causal=False, keep=None, p=0.0):
    """the packed in-projection form: qkv (B, L, 3, H, E) -> (O (B, L, H, E), dqkv (B, L, 3, H, E))"""
    qkv = _f64(qkv)
    out, dq, dk, dv = attention_forward_backward(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], upstream, scale, causal, keep, p)
    return out, torch.stack([dq, dk, dv], dim=2)


def shared_kv_forward_backward(q, k, v, upstream, scale, keep=None, p=0.0):
    """one key / value set for the whole batch: q (B, L, H, E), k (S, H, E), v (S, H, D); keep (H, B L, S) -- the scores of this form
    live as (H, B L, S), element (h B L + b L + l) S + s of the flat mask.  -> (O (B, L, H, D), dq, dk (S, H, E), dv (S, H, D))"""
    q, k, v = (_f64(t).clone().requires_grad_(True) for t in (q, k, v))
    B, L, H, _ = q.shape
    S = k.shape[0]
    if keep is not None:
        keep = _f64(keep).view(H, B, L, S).permute(1, 0, 2, 3)
    out, _ = attention(q, k.unsqueeze(0).expand(B, -1, -1, -1), v.unsqueeze(0).expand(B, -1, -1, -1), scale, False, keep, p)
    (out * _f64(upstream)).sum().backward()
    return out.detach(), q.grad.detach(), k.grad.detach(), v.grad.detach()
