"""float64 restatement of TimeLLM's frozen BERT body over [prefix | tail] -- BertModel(inputs_embeds=cat([prefix, tail], 1))
.last_hidden_state[:, -S_t:] with token type 0, absolute positions and NO attention mask -- and its gradient with respect to the tail.
The layers are those of tests/bert_embed_ref.py (`body`) started from embeddings instead of token ids, over a dense batch; autograd over
float64 torch ops gives the gradient.  Attention is bidirectional, so the tail's gradient flows through the prefix rows of every layer
but the last.  Optional keep-masks restate training mode's four dropouts (the embedding's, behind its LayerNorm; the attention
probabilities'; the two hidden dropouts of each layer, on the branch in front of the add + LayerNorm)."""
import math

import torch

from bert_embed_ref import _lin, _ln, build_bert, weights64  # noqa: F401


def _drop(x, keep, p):
    """x with the elements whose keep-mask is 0 dropped and the rest scaled by 1 / (1 - p); keep None: x"""
    if keep is None:
        return x
    return x * keep.to(x.dtype) / (1.0 - p)


def embed(w, x, eps, keep=None, p_h=0.0):
    """x (B, S, d) input embeddings -> the embedding stage's output: dropout(LayerNorm(x + pos[0:S] + type[0]))"""
    e = "embeddings."
    x = x + w[e + "position_embeddings.weight"][:x.shape[1]] + w[e + "token_type_embeddings.weight"][0]
    return _drop(_ln(x, w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps), keep, p_h)


def layer(w, x, i, n_head, eps, keeps=(None, None, None), p_h=0.0, p_a=0.0):
    """one post-LN encoder layer over (B, S, d); keeps: (attn (B, H, S, S), hid1 (B, S, d), hid2 (B, S, d)) keep-masks or None"""
    B, S, d = x.shape
    hd = d // n_head
    k_attn, k_h1, k_h2 = keeps
    p = f"encoder.layer.{i}."
    q, k, v = (_lin(x, w, p + "attention.self." + n).view(B, S, n_head, hd).transpose(1, 2) for n in ("query", "key", "value"))
    prob = _drop(torch.softmax(q @ k.transpose(2, 3) / math.sqrt(hd), dim=-1), k_attn, p_a)      # every query sees every key
    ctx = (prob @ v).transpose(1, 2).reshape(B, S, d)
    x = _ln(_drop(_lin(ctx, w, p + "attention.output.dense"), k_h1, p_h) + x, w[p + "attention.output.LayerNorm.weight"],
            w[p + "attention.output.LayerNorm.bias"], eps)
    h = _lin(x, w, p + "intermediate.dense")
    h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    return _ln(_drop(_lin(h, w, p + "output.dense"), k_h2, p_h) + x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps)


def hidden(w, x, n_layer, n_head, eps, masks=None):
    """x (B, S, d) float64 input embeddings -> the last hidden state (B, S, d); differentiable in x.
    masks: None, or dict(p_hidden, p_attn, embd (B, S, d), layers = [(attn (B, H, S, S), hid1 (B, S, d), hid2 (B, S, d)), ...])"""
    m = masks or {}
    p_h, p_a = m.get("p_hidden", 0.0), m.get("p_attn", 0.0)
    x = embed(w, x, eps, m.get("embd"), p_h)
    for i in range(n_layer):
        x = layer(w, x, i, n_head, eps, m["layers"][i] if masks else (None, None, None), p_h, p_a)
    return x


def tail_forward_backward(w, prefix, tail, upstream, n_layer, n_head, eps, masks=None):
    """(out (B, S_t, d), d tail (B, S_t, d)) in float64 for the loss sum(out * upstream); the prefix is a constant"""
    prefix = prefix.detach().double()
    tail = tail.detach().double().clone().requires_grad_(True)
    S_t = tail.shape[1]
    out = hidden(w, torch.cat([prefix, tail], 1), n_layer, n_head, eps, masks)[:, -S_t:]
    (out * upstream.double()).sum().backward()
    return out.detach(), tail.grad.detach()
