"""Plain-torch float64 restatement of the frozen GPT-2 body as transformers' GPT2Model(inputs_embeds=...) computes it (modeling_gpt2.py:
GPT2Model.forward, GPT2Block, GPT2Attention + eager_attention_forward, GPT2MLP), with explicit keep-masks for its three kinds of
dropout, and its full backward through autograd.  tests/test_gpt2_ref.py pins it to the installed GPT2Model on the CPU; the GPU tests
compare immtsf.ops.gpt2_body with it.

    x = drop_e(inputs + wpe[0:S])
    per block:  x = x + drop_r1(c_proj(softmax_causal(q k^T / sqrt(hd)) -> drop_a -> @ v))      q | k | v = c_attn(ln_1 x)
                x = x + drop_r2(c_proj(gelu_new(c_fc(ln_2 x))))
    ln_f(x)

Conv1D weights are (in, out).  masks: None (no dropout) or {"p": (p_embd, p_attn, p_resid), "embd": (B, S, d), "attn": [per layer
(B, H, S, S)], "resid1" / "resid2": [per layer (B, S, d)]} of 0 / 1 keep flags; a kept element is scaled by 1 / (1 - p)."""
import math

import torch
import torch.nn.functional as F


def weights64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _drop(x, mask, p):
    return x if mask is None or p <= 0.0 else x * mask.to(x.dtype) / (1.0 - p)


def body(w, inputs, n_layer, n_head, eps=1e-5, masks=None):
    """inputs (B, S, d) float64 -> ln_f output (B, S, d)"""
    B, S, d = inputs.shape
    hd = d // n_head
    p_e, p_a, p_r = masks["p"] if masks else (0.0, 0.0, 0.0)
    m = (lambda kind, i=None: None) if masks is None else (lambda kind, i=None: masks[kind] if i is None else masks[kind][i])
    x = _drop(inputs + w["wpe.weight"][:S], m("embd"), p_e)
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    for i in range(n_layer):
        g = lambda k: w[f"h.{i}.{k}"]      # noqa: E731
        h = F.layer_norm(x, (d,), g("ln_1.weight"), g("ln_1.bias"), eps)
        q, k, v = (h @ g("attn.c_attn.weight") + g("attn.c_attn.bias")).split(d, dim=2)
        q, k, v = (t.view(B, S, n_head, hd).transpose(1, 2) for t in (q, k, v))
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
        sc = sc.masked_fill(~causal, float("-inf"))
        a = _drop(torch.softmax(sc, dim=-1), m("attn", i), p_a)
        o = (a @ v).transpose(1, 2).reshape(B, S, d)
        x = x + _drop(o @ g("attn.c_proj.weight") + g("attn.c_proj.bias"), m("resid1", i), p_r)
        h = F.layer_norm(x, (d,), g("ln_2.weight"), g("ln_2.bias"), eps)
        h = gelu_new(h @ g("mlp.c_fc.weight") + g("mlp.c_fc.bias"))
        x = x + _drop(h @ g("mlp.c_proj.weight") + g("mlp.c_proj.bias"), m("resid2", i), p_r)
    return F.layer_norm(x, (d,), w["ln_f.weight"], w["ln_f.bias"], eps)


def tail_forward_backward(w, prefix, tail, upstream, n_layer, n_head, eps=1e-5, masks=None):
    """-> (hidden_tail (B, S_t, d), d tail) for the loss sum(hidden_tail * upstream): the FULL backward over all rows, of which the tail
    slice is returned"""
    tail = tail.detach().double().clone().requires_grad_(True)
    full = tail if prefix is None or prefix.shape[1] == 0 else torch.cat([prefix.detach().double(), tail], dim=1)
    out = body(w, full, n_layer, n_head, eps, masks)[:, -tail.shape[1]:]
    (out * upstream.double()).sum().backward()
    return out.detach(), tail.grad.detach()
