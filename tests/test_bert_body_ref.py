"""CPU pin of tests/bert_body_ref.py, the float64 restatement the GPU tests of immtsf.ops.bert_body are measured against, to
transformers' own BertModel(inputs_embeds=cat([prefix, tail], 1)).double() on the CPU in eval mode: the tail's last hidden state and the
gradient the tail takes from a loss over it (a random upstream: the sum of a LayerNorm output with unit gain is constant), at the
shapes of tests/test_gpu_bert_body.py, for 1, 2 and 3 layers.  Both are float64 and the same arithmetic: 1e-10 of the largest element.
The dependency the body's backward rests on is checked too: BERT is bidirectional, so -- unlike the GPT-2 and Llama bodies -- a loss over
the PREFIX rows' outputs gives the tail a non-zero gradient, and with two or more layers the tail's gradient changes when the prompt rows
are cut out of the graph behind the first layer.  Last, models/TimeLLM.py builds its offline BERT stand-in (no GPU needed for that)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_body_ref as R  # noqa: E402

N_POS, VOCAB = 96, 50
BODIES = {"a": dict(n_head=2, hidden=128, inner=256), "b": dict(n_head=3, hidden=192, inner=384)}
SHAPES = [(3, 37, 5), (2, 0, 33), (1, 1, 1), (2, 60, 4), (2, 17, 40), (1, 31, 65)]


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def _inputs(shape, d):
    B, S_p, S_t = shape
    g = torch.Generator().manual_seed(100 + 7 * B + S_p + 3 * S_t)
    return tuple(torch.randn(B, n, d, generator=g, dtype=torch.float64) for n in (S_p, S_t, S_t))


def _build(body, n_layer):
    b = BODIES[body]
    return R.build_bert(None, VOCAB, n_layer, b["hidden"], b["n_head"], b["inner"], N_POS).requires_grad_(False)


@pytest.mark.parametrize("n_layer", [1, 2, 3])
@pytest.mark.parametrize("body,shape", [("a", s) for s in SHAPES] + [("b", (3, 37, 5)), ("b", (2, 17, 40))],
                         ids=[f"a_B{s[0]}_Sp{s[1]}_St{s[2]}" for s in SHAPES] + ["b_B3_Sp37_St5", "b_B2_Sp17_St40"])
def test_restatement_equals_transformers(body, shape, n_layer):
    b = BODIES[body]
    model = _build(body, n_layer)
    w = R.weights64(model)
    eps = model.config.layer_norm_eps
    prefix, tail, up = _inputs(shape, b["hidden"])
    S_t = shape[2]
    model = model.double().eval()
    t2 = tail.clone().requires_grad_(True)
    hf = model(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, -S_t:]
    (hf * up).sum().backward()
    out, grad = R.tail_forward_backward(w, prefix, tail, up, n_layer, b["n_head"], eps)
    eo, eg = _rel(out, hf.detach()), _rel(grad, t2.grad)
    print(f"{body} {shape} L{n_layer}: out {eo:.2e}  d tail {eg:.2e}")
    assert out.shape == (shape[0], S_t, b["hidden"])
    assert float(t2.grad.abs().max()) > 0
    assert eo < 1e-10 and eg < 1e-10


def test_the_tail_gradient_flows_through_the_prompt_rows():
    b = BODIES["a"]
    model = _build("a", 2)
    w = R.weights64(model)
    eps = model.config.layer_norm_eps
    prefix, tail, up = _inputs((3, 37, 5), b["hidden"])
    S_p = 37
    g = torch.Generator().manual_seed(9)
    up_p = torch.randn(prefix.shape, generator=g, dtype=torch.float64)
    t1 = tail.clone().requires_grad_(True)
    (R.hidden(w, torch.cat([prefix, t1], 1), 2, b["n_head"], eps)[:, :S_p] * up_p).sum().backward()
    assert float(t1.grad.abs().max()) > 0                      # a prefix row's output depends on the tail rows
    _, grad = R.tail_forward_backward(w, prefix, tail, up, 2, b["n_head"], eps)
    # the same loss with the prompt rows of the first layer's output held constant: what a tail-rows-only backward would compute
    t3 = tail.clone().requires_grad_(True)
    x1 = R.layer(w, R.embed(w, torch.cat([prefix, t3], 1), eps), 0, b["n_head"], eps)
    x = R.layer(w, torch.cat([x1[:, :S_p].detach(), x1[:, S_p:]], 1), 1, b["n_head"], eps)
    out_cut = x[:, S_p:]
    (out_cut * up).sum().backward()
    out, _ = R.tail_forward_backward(w, prefix, tail, up, 2, b["n_head"], eps)
    assert _rel(out_cut.detach(), out) < 1e-12                 # the same forward ...
    assert _rel(t3.grad, grad) > 1e-3                          # ... but not the same gradient: the prompt rows carry part of it


def test_masks_of_ones_change_nothing_and_a_dropped_element_does():
    b = BODIES["a"]
    model = _build("a", 2)
    w = R.weights64(model)
    eps = model.config.layer_norm_eps
    B, S_p, S_t = 2, 17, 40
    S, H, d = S_p + S_t, b["n_head"], b["hidden"]
    prefix, tail, up = _inputs((B, S_p, S_t), d)
    out, grad = R.tail_forward_backward(w, prefix, tail, up, 2, H, eps)
    ones = lambda *s: torch.ones(*s, dtype=torch.uint8)       # noqa: E731
    masks = dict(p_hidden=0.0, p_attn=0.0, embd=ones(B, S, d), layers=[(ones(B, H, S, S), ones(B, S, d), ones(B, S, d)) for _ in range(2)])
    out1, grad1 = R.tail_forward_backward(w, prefix, tail, up, 2, H, eps, masks)
    assert torch.equal(out, out1) and torch.equal(grad, grad1)
    masks["p_hidden"] = masks["p_attn"] = 0.3
    masks["layers"][0][0][0, 0, 0, 0] = 0                      # one probability of a prefix query in the first layer
    out2, _ = R.tail_forward_backward(w, prefix, tail, up, 2, H, eps, masks)
    assert _rel(out2, out) > 1e-6


def test_timellm_builds_the_offline_bert_stand_in():
    from models.TimeLLM import TimeLLM
    stand_in = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, vocab_size=320, max_position_embeddings=1024)
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="BERT", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device="cpu", immtsf_offline_llm=stand_in)
    torch.manual_seed(0)
    m = TimeLLM(cfg)
    assert type(m.llm_model).__name__ == "BertModel" and m.d_llm == 128 and len(m.llm_model.encoder.layer) == 2
    assert not any(p.requires_grad for p in m.llm_model.parameters())
    assert m.word_embeddings.shape == (320, 128) and m.fused_body_calls == 0
    assert any(k.startswith("llm_model.encoder.layer.1.") for k in m.state_dict())
    cfg.immtsf_offline_llm = dict(stand_in, vocab_size=100)
    with pytest.raises(ValueError):
        TimeLLM(cfg)
