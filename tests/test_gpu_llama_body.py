"""GPU checks of TimeLLM's frozen Llama body: immtsf.ops.llama_body (csrc/llama_body.hip, the forward row kernels of csrc/llama_embed.hip
and the GEMM family) against the float64 restatement tests/llama_body_ref.py (pinned to transformers on the CPU in
tests/test_llama_body_ref.py), and models/TimeLLM.py through forecasting().
Bodies, as in tests/test_gpu_llama_embed.py, head_dim 128, max_position_embeddings 96:
  a: 2 heads over 1 K/V head (G = 2), 256 wide, intermediate 512, llama3 RoPE;  b: 2 over 2 (G = 1), default RoPE;
  c: 4 heads over 1 (G = 4), 512 wide, intermediate 384, llama3 RoPE
Shapes (B, S_p, S_t), 2 layers unless marked: (3, 37, 5) tail inside the second 32-tile; (2, 0, 33) no prefix, the tail crosses a tile
edge; (1, 1, 1); (2, 60, 4) tail straddles row 64; (2, 17, 40) tail longer than the prefix, two query tiles, dK / dV across tiles;
(1, 31, 65) S at the position limit, three tiles; (3, 37, 5) with 1 layer: the first block is also the q_from block.
Bars, relative to the largest element: fp32 mode 1e-4 for the output and 3e-4 for the gradient; bf16 mode 4x the error,
against float64, of transformers' own body under torch.autocast(bfloat16) on the same inputs (measured per case, printed)."""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_body_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_BAR, GRAD_BAR = 1e-4, 3e-4
N_POS, VOCAB = 96, 50
BODIES = {"a": dict(n_head=2, n_kv=1, hidden=256, inner=512, rope=R.LLAMA3_ROPE),
          "b": dict(n_head=2, n_kv=2, hidden=256, inner=512, rope=R.DEFAULT_ROPE),
          "c": dict(n_head=4, n_kv=1, hidden=512, inner=384, rope=R.LLAMA3_ROPE)}
SHAPES = [(3, 37, 5), (2, 0, 33), (1, 1, 1), (2, 60, 4), (2, 17, 40), (1, 31, 65)]
SHAPE_CASES = [(s, 2) for s in SHAPES] + [((3, 37, 5), 1)]       # (B, S_p, S_t), n_layer
CASES = [(b, s, n) for b in BODIES for s, n in SHAPE_CASES]
IDS = [f"{b}_B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for b, s, n in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(body, n_layer):
    return R.build_llama(None, VOCAB, n_layer, max_pos=N_POS, head_dim=128, **BODIES[body]).requires_grad_(False).to(_dev())


@functools.lru_cache(maxsize=None)
def _inputs(shape, d):
    B, S_p, S_t = shape
    g = torch.Generator().manual_seed(100 + 7 * B + S_p + 3 * S_t)
    return tuple(torch.randn(B, n, d, generator=g) for n in (S_p, S_t, S_t))       # prefix, tail, upstream


@functools.lru_cache(maxsize=None)
def _reference(body, shape, n_layer):
    """float64, computed once, shared"""
    m, b = _model(body, n_layer), BODIES[body]
    prefix, tail, up = _inputs(shape, b["hidden"])
    return R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, b["n_head"], b["n_kv"], m.config.rms_norm_eps)


def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def _fused(body, shape, n_layer, precision, prefix_grad=False):
    from immtsf import ops
    dev = _dev()
    prefix, tail, up = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
    tail = tail.clone().requires_grad_(True)
    prefix = prefix.clone().requires_grad_(prefix_grad)
    out = ops.llama_body(_model(body, n_layer), prefix, tail, False, precision=precision)
    (out * up).sum().backward()
    return out.detach(), tail.grad.detach(), prefix


@pytest.mark.parametrize("body,shape,n_layer", CASES, ids=IDS)
def test_fp32_against_float64(body, shape, n_layer):
    out, grad, _ = _fused(body, shape, n_layer, "fp32")
    want_out, want_grad = _reference(body, shape, n_layer)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{body} {shape} L{n_layer}: out {eo:.2e} (bar {OUT_BAR:.0e})  d tail {eg:.2e} (bar {GRAD_BAR:.0e})")
    assert out.shape == (shape[0], shape[2], BODIES[body]["hidden"]) and out.dtype == torch.float32
    assert eo < OUT_BAR and eg < GRAD_BAR


@pytest.mark.parametrize("body,shape,n_layer", CASES, ids=IDS)
def test_bf16_within_4x_of_autocast(body, shape, n_layer):
    dev = _dev()
    m = _model(body, n_layer)
    want_out, want_grad = _reference(body, shape, n_layer)
    prefix, tail, up = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
    t2 = tail.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        hf = m(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, -shape[2]:]
    (hf.float() * up).sum().backward()
    ho, hg = _rel(hf.float(), want_out), _rel(t2.grad, want_grad)
    out, grad, _ = _fused(body, shape, n_layer, "bf16")
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{body} {shape} L{n_layer} bf16: out {eo:.2e} (autocast {ho:.2e})  d tail {eg:.2e} (autocast {hg:.2e})")
    assert eo <= 4.0 * ho and eg <= 4.0 * hg


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_runs_give_the_same_bits_and_no_grad_gives_the_same_output(precision):
    from immtsf import ops
    dev = _dev()
    for body, shape in (("a", (2, 17, 40)), ("c", (3, 37, 5))):
        a = _fused(body, shape, 2, precision)
        b = _fused(body, shape, 2, precision)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        prefix, tail, _ = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
        with torch.no_grad():
            out = ops.llama_body(_model(body, 2), prefix, tail.clone().requires_grad_(True), False, precision=precision)
        assert out.grad_fn is None and not out.requires_grad
        assert torch.equal(out, a[0])


def test_prefix_may_require_grad_and_gets_none():
    _, grad, _ = _fused("a", (3, 37, 5), 2, "fp32")
    _, grad_p, prefix = _fused("a", (3, 37, 5), 2, "fp32", prefix_grad=True)
    assert prefix.requires_grad and prefix.grad is None
    assert torch.equal(grad, grad_p)


def test_supported_limits():
    import note_embed_ref as NR

    from immtsf import ops
    dev = _dev()
    for body in BODIES:
        assert ops.llama_body_supported(_model(body, 2), 37, 5) and ops.llama_body_supported(_model(body, 2), 0, N_POS)
        assert ops.llama_body_supported(_model(body, 2), 95, 1)
    assert not ops.llama_body_supported(_model("a", 2), 92, 5)                       # S past max_position_embeddings
    assert not ops.llama_body_supported(_model("a", 2), 37, 0)                       # no tail
    assert not ops.llama_body_supported(_model("a", 2), -1, 5)
    assert not ops.llama_body_supported(torch.nn.Linear(4, 4), 37, 5)

    def build(**kw):
        args = dict(n_head=2, n_kv=1, hidden=256, inner=512, head_dim=128, rope=R.DEFAULT_ROPE)
        args.update(kw)
        return R.build_llama(None, VOCAB, 1, max_pos=N_POS, **args).to(dev)

    bad = [build(hidden=128, head_dim=64), build(n_head=3, hidden=384), build(hidden_act="gelu"),
           build(rope={"rope_type": "dynamic", "rope_theta": 10000.0, "factor": 2.0}), build().to(torch.bfloat16),
           build(attention_bias=True), NR.build_model(None, VOCAB, 1, 128, 2, N_POS).to(dev)]
    assert ops.llama_body_supported(build(), 3, 5)
    for m in bad:
        assert not ops.llama_body_supported(m, 3, 5)
        d = m.config.hidden_size
        with pytest.raises(Exception):
            ops.llama_body(m, torch.zeros(1, 3, d, device=dev), torch.zeros(1, 5, d, device=dev), False)
    with pytest.raises(Exception):
        ops.llama_body(_model("a", 2), torch.zeros(1, 92, 256, device=dev), torch.zeros(1, 5, 256, device=dev), False)
    with pytest.raises(Exception):              # attention dropout in training mode: the caller takes the stock path
        ops.llama_body(build(attention_dropout=0.1), torch.zeros(1, 3, 256, device=dev), torch.zeros(1, 5, 256, device=dev), True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_raw_text_path_keeps_its_bits(precision):
    """llama_embed_notes and llama_body share the weight caches on the model"""
    from immtsf import ops
    dev = _dev()
    m = _model("a", 2)
    g = torch.Generator().manual_seed(5)
    counts = (3, 33, 0, 64)
    ids = torch.randint(0, VOCAB, (sum(counts),), generator=g).to(torch.int32).to(dev)
    cu = torch.tensor([0, 3, 36, 36, 100], dtype=torch.int32, device=dev)
    before = ops.llama_embed_notes(m, ids, cu, precision=precision)
    _fused("a", (3, 37, 5), 2, precision)
    after = ops.llama_embed_notes(m, ids, cu, precision=precision)
    assert torch.equal(before, after) and torch.isfinite(after).all()


# ---- TimeLLM through the front door -------------------------------------------------------------------------------------------------------
def _timellm(dev, **llama):
    from models.TimeLLM import TimeLLM
    stand_in = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, intermediate_size=512, vocab_size=320)
    stand_in.update(llama)
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="LLAMA", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device=str(dev), immtsf_offline_llm=stand_in)
    torch.manual_seed(0)
    m = TimeLLM(cfg).to(dev).train()
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    g = torch.Generator().manual_seed(1)
    data = torch.randn(3, 12, 3, generator=g).to(dev)
    mask = (torch.rand(3, 12, 3, generator=g) < 0.8).float().to(dev)
    tp = torch.sort(torch.rand(3, 12, generator=g), 1).values.to(dev)
    return m, (torch.rand(3, 5, generator=g).to(dev), data * mask, tp, mask)


def _run(m, batch, fused):
    from immtsf import config
    was, was_p = config.timellm_fused, config.precision
    config.timellm_fused, config.precision = fused, "fp32"
    try:
        config.manual_seed(7)            # the reprogramming layer's attention dropout: the same keys in both runs
        m.zero_grad(set_to_none=True)
        out = m.forecasting(*batch)
        out.square().mean().backward()
    finally:
        config.timellm_fused, config.precision = was, was_p
    return out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.requires_grad}


def test_timellm_takes_the_fused_llama_body_and_equals_the_stock_call():
    dev = _dev()
    m, batch = _timellm(dev)
    assert type(m.llm_model).__name__ == "LlamaModel" and m.d_llm == 256 and len(m.llm_model.layers) == 2
    assert m.llm_model.training and not any(p.requires_grad for p in m.llm_model.parameters())
    out, grads = _run(m, batch, True)
    assert m.fused_body_calls == 1
    want, want_grads = _run(m, batch, False)
    assert m.fused_body_calls == 1                      # the stock run leaves the counter alone
    assert out.shape == (3, 5, 3) and torch.isfinite(out).all()
    eo = _rel(out, want)
    print(f"TimeLLM (Llama stand-in) fused vs stock: out {eo:.2e}")
    assert eo < OUT_BAR
    assert set(grads) == set(want_grads) and len(grads) > 0
    # the error of a gradient is taken relative to the largest gradient element of the parameter's own layer (weight and bias together):
    # the reprogramming layer's key bias shifts every score of a query by the same amount, so its true gradient is 0 -- both runs give
    # rounding noise of the sums that also form the weight's gradient, and that noise has no scale of its own
    scale = {}
    for k, g in want_grads.items():
        owner = k.rsplit(".", 1)[0]
        scale[owner] = max(scale.get(owner, 0.0), float(g.abs().max()))
    for k in grads:
        eg = float((grads[k] - want_grads[k]).abs().max()) / scale[k.rsplit(".", 1)[0]]
        print(f"  d {k}: {eg:.2e}")
        assert eg < GRAD_BAR, k


def test_timellm_with_attention_dropout_in_training_takes_the_stock_path():
    dev = _dev()
    m, batch = _timellm(dev, attention_dropout=0.1)
    assert m.llm_model.training and m.llm_model.config.attention_dropout == 0.1
    out, _ = _run(m, batch, True)
    assert m.fused_body_calls == 0 and torch.isfinite(out).all()
    m.llm_model.eval()
    _run(m, batch, True)
    assert m.fused_body_calls == 1
