"""CPU pin of tests/llama_body_ref.py, the float64 restatement the GPU tests of immtsf.ops.llama_body are measured against, to
transformers' own LlamaModel(inputs_embeds=cat([prefix, tail], 1)) on the CPU: the tail's last hidden state and the gradient the tail
takes from a loss over it, at the shapes of tests/test_gpu_llama_body.py, for G = 2 with llama3 RoPE and G = 1 with default RoPE.
Bars as in tests/test_llama_embed_ref.py: LlamaModel.double() takes its rotary angles and every RMSNorm row in fp32, so with the
restatement following both (norm32) the two are the same arithmetic and must agree at 1e-10 of the largest element; with float64 norms
-- the form the kernels are measured against -- it stays within fp32 rounding of that, 1e-5.
The exactness claim the tail-only backward rests on is checked on both: no prefix row depends on a tail row, i.e. a loss over the PREFIX
rows' outputs gives the tail an exact zero gradient (so the full backward's work on the prefix rows contributes nothing to d tail), and
the fused op, which detaches the prefix, loses nothing of d tail.  (A prefix that itself required a gradient would take a non-zero one
from the tail's loss through its keys and values; TimeLLM's prefix is the frozen embedding of the prompt, and llama_body gives it none.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_body_ref as R  # noqa: E402

N_LAYER, N_POS, VOCAB = 2, 96, 50
BODIES = {"a": dict(n_head=2, n_kv=1, hidden=256, inner=512, rope=R.LLAMA3_ROPE),
          "b": dict(n_head=2, n_kv=2, hidden=256, inner=512, rope=R.DEFAULT_ROPE)}
SHAPES = [(3, 37, 5), (2, 0, 33), (1, 1, 1), (2, 60, 4), (2, 17, 40), (1, 31, 65)]


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def _inputs(shape, d):
    B, S_p, S_t = shape
    g = torch.Generator().manual_seed(100 + 7 * B + S_p + 3 * S_t)
    return tuple(torch.randn(B, n, d, generator=g, dtype=torch.float64) for n in (S_p, S_t, S_t))


@pytest.mark.parametrize("body", list(BODIES))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{s[0]}_Sp{s[1]}_St{s[2]}" for s in SHAPES])
def test_restatement_equals_transformers(body, shape):
    b = BODIES[body]
    model = R.build_llama(None, VOCAB, N_LAYER, max_pos=N_POS, head_dim=128, **b).requires_grad_(False)
    w = R.weights64(model)
    eps = model.config.rms_norm_eps
    prefix, tail, up = _inputs(shape, b["hidden"])
    S_t = shape[2]
    model = model.double()
    t2 = tail.clone().requires_grad_(True)
    hf = model(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, -S_t:]
    (hf * up).sum().backward()
    out, grad = R.tail_forward_backward(w, prefix, tail, up, N_LAYER, b["n_head"], b["n_kv"], eps, norm32=True)
    out64, grad64 = R.tail_forward_backward(w, prefix, tail, up, N_LAYER, b["n_head"], b["n_kv"], eps)
    eo, eg = _rel(out, hf.detach()), _rel(grad, t2.grad)
    eo64, eg64 = _rel(out64, hf.detach()), _rel(grad64, t2.grad)
    print(f"{body} {shape}: out {eo:.2e}  d tail {eg:.2e}; with float64 norms out {eo64:.2e}  d tail {eg64:.2e}")
    assert out.shape == (shape[0], S_t, b["hidden"])
    assert eo < 1e-10 and eg < 1e-10
    assert eo64 < 1e-5 and eg64 < 1e-5


@pytest.mark.parametrize("shape", [(3, 37, 5), (2, 17, 40)], ids=["B3_Sp37_St5", "B2_Sp17_St40"])
def test_no_prefix_row_depends_on_a_tail_row(shape):
    b = BODIES["a"]
    model = R.build_llama(None, VOCAB, N_LAYER, max_pos=N_POS, head_dim=128, **b).requires_grad_(False)
    w = R.weights64(model)
    prefix, tail, up = _inputs(shape, b["hidden"])
    S_p = shape[1]
    g = torch.Generator().manual_seed(9)
    up_p = torch.randn(prefix.shape, generator=g, dtype=torch.float64)
    # the restatement: a loss over the prefix rows' outputs
    t1 = tail.clone().requires_grad_(True)
    (R.hidden(w, torch.cat([prefix, t1], 1), N_LAYER, b["n_head"], b["n_kv"], model.config.rms_norm_eps)[:, :S_p] * up_p).sum().backward()
    assert torch.equal(t1.grad, torch.zeros_like(t1.grad))
    # transformers' own body
    t2 = tail.clone().requires_grad_(True)
    (model.double()(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, :S_p] * up_p).sum().backward()
    assert torch.equal(t2.grad, torch.zeros_like(t2.grad))
    # so the tail's gradient is the same whether or not the prefix is part of the graph (what the fused op's detach relies on)
    _, g_det = R.tail_forward_backward(w, prefix, tail, up, N_LAYER, b["n_head"], b["n_kv"], model.config.rms_norm_eps)
    _, g_att, g_pre = R.tail_forward_backward(w, prefix, tail, up, N_LAYER, b["n_head"], b["n_kv"], model.config.rms_norm_eps, prefix_grad=True)
    assert torch.equal(g_det, g_att) and g_pre.abs().max() > 0
