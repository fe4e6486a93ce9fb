"""float64 restatement of TimeLLM's frozen Llama body over [prefix | tail] -- LlamaModel(inputs_embeds=cat([prefix, tail], 1))
.last_hidden_state[:, -S_t:] -- and its gradient with respect to the tail (and, to show that it is zero, the prefix is NOT an input of the
tail's backward: see tests/test_llama_body_ref.py).  The layers are those of tests/llama_embed_ref.py (`body`) started from embeddings
instead of token ids; autograd over float64 torch ops gives the gradient.  As there, the rotary angles are fp32 values (transformers
forms them in fp32 in a model of any dtype) and the norms are float64 unless norm32 asks for transformers' fp32 rows."""
import math

import torch

from llama_embed_ref import DEFAULT_ROPE, LLAMA3_ROPE, _rms, _rotate, build_llama, rope_tables, weights64  # noqa: F401


def hidden(w, x, n_layer, n_head, n_kv, eps, norm32=False):
    """x (B, S, d) float64 input embeddings -> the last hidden state (B, S, d) after the final norm; differentiable in x"""
    B, S, _ = x.shape
    hd = w["layers.0.self_attn.q_proj.weight"].shape[0] // n_head
    cos, sin = rope_tables(w, S)
    causal = torch.full((S, S), float("-inf"), dtype=torch.float64).triu(1)
    for i in range(n_layer):
        p = f"layers.{i}."
        h = _rms(x, w[p + "input_layernorm.weight"], eps, norm32)
        q = (h @ w[p + "self_attn.q_proj.weight"].T).view(B, S, n_head, hd).transpose(1, 2)
        k = (h @ w[p + "self_attn.k_proj.weight"].T).view(B, S, n_kv, hd).transpose(1, 2)
        v = (h @ w[p + "self_attn.v_proj.weight"].T).view(B, S, n_kv, hd).transpose(1, 2)
        q, k = _rotate(q, cos, sin), _rotate(k, cos, sin)
        k, v = (t.repeat_interleave(n_head // n_kv, dim=1) for t in (k, v))          # query head h reads K/V head h // G
        prob = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(hd) + causal, dim=-1)
        x = x + (prob @ v).transpose(1, 2).reshape(B, S, n_head * hd) @ w[p + "self_attn.o_proj.weight"].T
        h = _rms(x, w[p + "post_attention_layernorm.weight"], eps, norm32)
        g = h @ w[p + "mlp.gate_proj.weight"].T
        x = x + (g * torch.sigmoid(g) * (h @ w[p + "mlp.up_proj.weight"].T)) @ w[p + "mlp.down_proj.weight"].T
    return _rms(x, w["norm.weight"], eps, norm32)


def tail_forward_backward(w, prefix, tail, upstream, n_layer, n_head, n_kv, eps, norm32=False, prefix_grad=False):
    """(out (B, S_t, d), d tail (B, S_t, d)[, d prefix]) in float64 for the loss sum(out * upstream)"""
    prefix = prefix.detach().double().clone().requires_grad_(prefix_grad)
    tail = tail.detach().double().clone().requires_grad_(True)
    S_t = tail.shape[1]
    out = hidden(w, torch.cat([prefix, tail], 1), n_layer, n_head, n_kv, eps, norm32)[:, -S_t:]
    (out * upstream.double()).sum().backward()
    if prefix_grad:
        return out.detach(), tail.grad.detach(), prefix.grad.detach()
    return out.detach(), tail.grad.detach()
