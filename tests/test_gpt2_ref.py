"""CPU checks behind the fused GPT-2 body: the float64 restatement (tests/gpt2_ref.py) equals the installed transformers GPT2Model, and
the causality claim the tail-only backward rests on holds."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpt2_ref as R  # noqa: E402


def _model(n_layer=2, **kw):
    from transformers import GPT2Config, GPT2Model
    torch.manual_seed(11)
    cfg = GPT2Config(n_embd=128, n_head=2, n_layer=n_layer, n_positions=64, vocab_size=32, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                     **kw)
    m = GPT2Model(cfg)
    with torch.no_grad():           # seeded weights away from the initialiser's zeros / ones, so that every bias and gain matters
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m.double().train()


@pytest.mark.parametrize("shape", [(3, 37, 5), (2, 0, 9), (1, 1, 1), (2, 17, 40)])
def test_restatement_equals_gpt2model(shape):
    B, S_p, S_t = shape
    m = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, S_p + S_t, 128, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(B, S_p + S_t, 128, generator=g, dtype=torch.float64)
    want = m(inputs_embeds=x).last_hidden_state
    (want * up).sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    got = R.body(R.weights64(m), x2, 2, 2, m.config.layer_norm_epsilon)
    (got * up).sum().backward()
    assert (got - want).abs().max() <= 1e-10 * want.abs().max()
    assert (x2.grad - x.grad).abs().max() <= 1e-10 * x.grad.abs().max()


@pytest.mark.parametrize("shape", [(3, 37, 5), (2, 17, 40)])
def test_tail_loss_gradient_needs_tail_rows_only(shape):
    """the causality claim: with a loss on the tail rows, cutting every gradient that reaches a prefix row (detaching the prefix rows
    of every block's input, hence their K, V, MLP and LayerNorm) leaves the tail rows' input gradient unchanged, because a prefix
    row's hidden state never depends on a tail row"""
    B, S_p, S_t = shape
    m = _model()
    w = R.weights64(m)
    g = torch.Generator().manual_seed(6)
    prefix = torch.randn(B, S_p, 128, generator=g, dtype=torch.float64)
    tail = torch.randn(B, S_t, 128, generator=g, dtype=torch.float64)
    up = torch.randn(B, S_t, 128, generator=g, dtype=torch.float64)
    _, want = R.tail_forward_backward(w, prefix, tail, up, 2, 2)

    # the same body with the prefix rows' path cut out of the graph at every block boundary
    import math
    import torch.nn.functional as F
    t = tail.clone().requires_grad_(True)
    S, d, H, hd = S_p + S_t, 128, 2, 64
    x = torch.cat([prefix, t], 1) + w["wpe.weight"][:S]
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    cut = lambda v: torch.cat([v[:, :S_p].detach(), v[:, S_p:]], 1)      # noqa: E731
    for i in range(2):
        p = lambda k: w[f"h.{i}.{k}"]      # noqa: E731
        x = cut(x)
        h = F.layer_norm(x, (d,), p("ln_1.weight"), p("ln_1.bias"))
        q, k, v = (cut(h) @ p("attn.c_attn.weight") + p("attn.c_attn.bias")).split(d, dim=2)
        q, k, v = (cut(u).view(B, S, H, hd).transpose(1, 2) for u in (q, k, v))
        sc = ((q @ k.transpose(-1, -2)) / math.sqrt(hd)).masked_fill(~causal, float("-inf"))
        o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, S, d)
        x = cut(x + o @ p("attn.c_proj.weight") + p("attn.c_proj.bias"))
        h = R.gelu_new(F.layer_norm(x, (d,), p("ln_2.weight"), p("ln_2.bias")) @ p("mlp.c_fc.weight") + p("mlp.c_fc.bias"))
        x = x + h @ p("mlp.c_proj.weight") + p("mlp.c_proj.bias")
    out = F.layer_norm(x, (d,), w["ln_f.weight"], w["ln_f.bias"])[:, S_p:]
    (out * up).sum().backward()
    assert (t.grad - want).abs().max() <= 1e-10 * want.abs().max()
    # and the prefix rows' hidden states do not move with the tail
    a = R.body(w, torch.cat([prefix, tail], 1), 2, 2)[:, :S_p]
    b = R.body(w, torch.cat([prefix, tail + 1.0], 1), 2, 2)[:, :S_p]
    assert torch.equal(a, b)
