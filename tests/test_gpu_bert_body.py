"""GPU checks of TimeLLM's frozen BERT body: immtsf.ops.bert_body (csrc/bert_body.hip, the erf GELU of csrc/bert_embed.hip and the GEMM
family) against the float64 restatement tests/bert_body_ref.py (pinned to transformers on the CPU in tests/test_bert_body_ref.py), and
models/TimeLLM.py through forecasting().
Bodies, head_dim 64, max_position_embeddings 96:  a: 2 heads, 128 wide, intermediate 256;  b: 3 heads, 192 wide, intermediate 384.
Shapes (B, S_p, S_t), 2 layers unless marked: (3, 37, 5) partial last key tile; (2, 0, 33) no prefix; (1, 1, 1); (2, 60, 4) S = 64
exactly, no partial tile; (2, 17, 40) tail longer than the prefix; (1, 31, 65) S at the position limit; (3, 37, 5) with 1 layer: both
reductions in one layer; (2, 17, 40) with 3 layers: a true middle layer whose backward covers all rows.  Any case with S_p > 0 and 2 or
more layers fails if the backward drops the prompt rows.
Bars, relative to the largest element: fp32 mode 1e-4 for the output and 3e-4 for the gradient, with and without dropout (the
masks rebuilt with ops.dropout_keep_mask and fed to the restatement); bf16 mode 4x the error, against float64, of transformers' own body
under torch.autocast(bfloat16) on the same inputs (measured per case, printed)."""
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_body_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_BAR, GRAD_BAR = 1e-4, 3e-4
N_POS, VOCAB, P_DROP, SEED = 96, 50, 0.3, 0x5EEDBE27
BODIES = {"a": dict(n_head=2, hidden=128, inner=256), "b": dict(n_head=3, hidden=192, inner=384)}
SHAPES = [(3, 37, 5), (2, 0, 33), (1, 1, 1), (2, 60, 4), (2, 17, 40), (1, 31, 65)]
SHAPE_CASES = [(s, 2) for s in SHAPES] + [((3, 37, 5), 1), ((2, 17, 40), 3)]       # (B, S_p, S_t), n_layer
CASES = [(b, s, n) for b in BODIES for s, n in SHAPE_CASES]
IDS = [f"{b}_B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for b, s, n in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(body, n_layer, p_drop=0.0):
    """the same weights at either dropout setting (the seed fixes them; the probabilities are config fields only)"""
    b = BODIES[body]
    return R.build_bert(None, VOCAB, n_layer, b["hidden"], b["n_head"], b["inner"], N_POS, hidden_dropout_prob=p_drop,
                        attention_probs_dropout_prob=p_drop).requires_grad_(False).to(_dev())


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
    return R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, b["n_head"], m.config.layer_norm_eps)


def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def _fused(body, shape, n_layer, precision, prefix_grad=False, p_drop=0.0):
    from immtsf import ops
    dev = _dev()
    prefix, tail, up = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
    tail = tail.clone().requires_grad_(True)
    prefix = prefix.clone().requires_grad_(prefix_grad)
    out = ops.bert_body(_model(body, n_layer, p_drop), prefix, tail, p_drop > 0.0, precision=precision, seed=SEED)
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


def _keep_masks(shape, n_layer, H, d):
    """the four sites' keep-masks as the kernels draw them, rebuilt from the seed, in the restatement's shapes (on the CPU)"""
    from immtsf import ops
    dev = _dev()
    B, S = shape[0], shape[1] + shape[2]
    rows = lambda site: ops.dropout_keep_mask(SEED, site, B * S * d, P_DROP, dev).view(B, S, d).cpu()       # noqa: E731
    layers = []
    for li in range(n_layer):
        s_attn, s_h1, s_h2 = ops.bert_sites(li)
        attn = ops.dropout_keep_mask(SEED, s_attn, B * H * S * 1024, P_DROP, dev).view(B, H, S, 1024)[..., :S].cpu()
        layers.append((attn, rows(s_h1), rows(s_h2)))
    return dict(p_hidden=P_DROP, p_attn=P_DROP, embd=rows(ops.BERT_SITE_EMBD), layers=layers)


@pytest.mark.parametrize("body,shape,n_layer", CASES, ids=IDS)
def test_dropout_masks_are_reproducible_and_the_masked_body_matches_float64(body, shape, n_layer):
    b = BODIES[body]
    m = _model(body, n_layer, P_DROP)
    assert m.config.hidden_dropout_prob == P_DROP and m.config.attention_probs_dropout_prob == P_DROP
    masks = _keep_masks(shape, n_layer, b["n_head"], b["hidden"])
    for name, k in [("embd", masks["embd"])] + [(f"L{i}.{n}", k) for i, ks in enumerate(masks["layers"])
                                                for n, k in zip(("attn", "hid1", "hid2"), ks)]:
        assert set(k.unique().tolist()) <= {0, 1}
        if k.numel() >= 4096:       # enough draws for the band: sigma = sqrt(0.21 / n) <= 0.0072 (the (1, 1, 1) case has 128 and 2)
            frac = float(k.float().mean())
            assert abs(frac - (1.0 - P_DROP)) < 0.05, (name, frac)
    prefix, tail, up = _inputs(shape, b["hidden"])
    want_out, want_grad = R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, b["n_head"], m.config.layer_norm_eps, masks)
    out, grad, _ = _fused(body, shape, n_layer, "fp32", p_drop=P_DROP)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    plain_out, _ = _reference(body, shape, n_layer)
    print(f"{body} {shape} L{n_layer} dropout {P_DROP}: out {eo:.2e} (bar {OUT_BAR:.0e})  d tail {eg:.2e} (bar {GRAD_BAR:.0e})")
    assert _rel(want_out, plain_out) > 1e-2                             # the masks do bite
    assert eo < OUT_BAR and eg < GRAD_BAR


@pytest.mark.parametrize("body,shape,n_layer", CASES, ids=IDS)
def test_bf16_within_4x_of_autocast(body, shape, n_layer):
    dev = _dev()
    m = _model(body, n_layer).eval()
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


@pytest.mark.parametrize("p_drop", [0.0, P_DROP], ids=["eval", "dropout"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_runs_give_the_same_bits_and_no_grad_gives_the_same_output(precision, p_drop):
    from immtsf import ops
    dev = _dev()
    for body, shape, n_layer in (("a", (2, 17, 40), 3), ("b", (3, 37, 5), 2)):
        a = _fused(body, shape, n_layer, precision, p_drop=p_drop)
        b = _fused(body, shape, n_layer, precision, p_drop=p_drop)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
        prefix, tail, _ = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
        with torch.no_grad():
            out = ops.bert_body(_model(body, n_layer, p_drop), prefix, tail.clone().requires_grad_(True), p_drop > 0.0, precision=precision,
                                seed=SEED)
        assert out.grad_fn is None and not out.requires_grad
        assert torch.equal(out, a[0])
        out = ops.bert_body(_model(body, n_layer, p_drop), prefix, tail, p_drop > 0.0, precision=precision, seed=SEED)
        assert out.grad_fn is None and torch.equal(out, a[0])      # a tail that needs no gradient: nothing saved either


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
        assert ops.bert_body_supported(_model(body, 2), 37, 5) and ops.bert_body_supported(_model(body, 2), 0, N_POS)
        assert ops.bert_body_supported(_model(body, 2), 95, 1)
    assert not ops.bert_body_supported(_model("a", 2), 92, 5)                       # S past max_position_embeddings
    assert not ops.bert_body_supported(_model("a", 2), 37, 0)                       # no tail
    assert not ops.bert_body_supported(_model("a", 2), -1, 5)
    assert not ops.bert_body_supported(torch.nn.Linear(4, 4), 37, 5)

    def build(hidden=128, n_head=2, **kw):
        return R.build_bert(None, VOCAB, 1, hidden, n_head, 256, N_POS, **kw).to(dev)

    bad = [build(n_head=4), build(hidden_act="gelu_new"), build(position_embedding_type="relative_key"), build().to(torch.bfloat16),
           NR.build_model(None, VOCAB, 1, 128, 2, N_POS).to(dev)]
    assert ops.bert_body_supported(build(), 3, 5)
    for m in bad:
        assert not ops.bert_body_supported(m, 3, 5)
        with pytest.raises(Exception):
            ops.bert_body(m, torch.zeros(1, 3, 128, device=dev), torch.zeros(1, 5, 128, device=dev), False)
    with pytest.raises(Exception):
        ops.bert_body(_model("a", 2), torch.zeros(1, 92, 128, device=dev), torch.zeros(1, 5, 128, device=dev), False)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_the_raw_text_path_keeps_its_bits(precision):
    """bert_embed_notes and bert_body share the weight caches on the model"""
    from immtsf import ops
    dev = _dev()
    m = _model("a", 2)
    g = torch.Generator().manual_seed(5)
    counts = (3, 33, 0, 64)
    ids = torch.randint(0, VOCAB, (sum(counts),), generator=g).to(torch.int32).to(dev)
    cu = torch.tensor([0, 3, 36, 36, 100], dtype=torch.int32, device=dev)
    before = ops.bert_embed_notes(m, ids, cu, precision=precision)
    _fused("a", (3, 37, 5), 2, precision)
    after = ops.bert_embed_notes(m, ids, cu, precision=precision)
    assert torch.equal(before, after) and torch.isfinite(after).all()


# ---- TimeLLM through the front door -------------------------------------------------------------------------------------------------------
def _timellm(dev):
    from models.TimeLLM import TimeLLM
    stand_in = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, vocab_size=320, max_position_embeddings=1024)
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="BERT", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device=str(dev), immtsf_offline_llm=stand_in)
    torch.manual_seed(0)
    m = TimeLLM(cfg).to(dev).eval()
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    g = torch.Generator().manual_seed(1)
    data = torch.randn(3, 12, 3, generator=g).to(dev)
    mask = (torch.rand(3, 12, 3, generator=g) < 0.8).float().to(dev)
    tp = torch.sort(torch.rand(3, 12, generator=g), 1).values.to(dev)
    return m, (torch.rand(3, 5, generator=g).to(dev), data * mask, tp, mask)


def _run(m, batch, fused, precision="fp32", bert_fp32=True):
    """bert_fp32: config.timellm_bert_fp32 -- fp32 mode takes the stock call by default (it measured faster); the knob routes
    it to the operator, which is how the two paths are compared at fp32 accuracy"""
    from immtsf import config
    was = config.timellm_fused, config.precision, config.timellm_bert_fp32
    config.timellm_fused, config.precision, config.timellm_bert_fp32 = fused, precision, bert_fp32
    try:
        m.zero_grad(set_to_none=True)
        out = m.forecasting(*batch)
        out.square().mean().backward()
    finally:
        config.timellm_fused, config.precision, config.timellm_bert_fp32 = was
    return out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.requires_grad}


def test_timellm_takes_the_fused_bert_body_and_equals_the_stock_call():
    dev = _dev()
    m, batch = _timellm(dev)
    assert type(m.llm_model).__name__ == "BertModel" and m.d_llm == 128 and len(m.llm_model.encoder.layer) == 2
    assert not m.llm_model.training and not any(p.requires_grad for p in m.llm_model.parameters())
    want, want_grads = _run(m, batch, False)
    assert m.fused_body_calls == 0                      # with the knob off the counter stays 0
    out, grads = _run(m, batch, True)
    assert m.fused_body_calls == 1
    assert out.shape == (3, 5, 3) and torch.isfinite(out).all()
    eo = _rel(out, want)
    print(f"TimeLLM (BERT stand-in) fused vs stock: out {eo:.2e}")
    assert eo < OUT_BAR
    assert set(grads) == set(want_grads) and len(grads) > 0
    # the error of a gradient is taken relative to the largest gradient element of the parameter's own layer (weight and bias together):
    # the reprogramming layer's key bias shifts every score of a query by the same amount, so its true gradient is 0 -- both runs give
    # rounding noise of the sums that also form the weight's gradient, and that noise has no scale of its own
    scale = {}
    for k, g in want_grads.items():
        owner = k.rsplit(".", 1)[0]
        scale[owner] = max(scale.get(owner, 0.0), float(g.abs().max()))
    checked = 0
    for k in grads:
        if k.startswith("reprogramming_layer.") or k.startswith("patch_embedding."):
            eg = float((grads[k] - want_grads[k]).abs().max()) / scale[k.rsplit(".", 1)[0]]
            print(f"  d {k}: {eg:.2e}")
            assert eg < GRAD_BAR, k
            checked += 1
    assert checked > 0


def test_timellm_dispatch_takes_the_bert_body_in_bf16_mode_and_the_stock_call_in_fp32_mode():
    dev = _dev()
    m, batch = _timellm(dev)
    out, _ = _run(m, batch, True, "fp32", bert_fp32=False)
    assert m.fused_body_calls == 0 and torch.isfinite(out).all()          # fp32 mode: the stock call, which measured faster
    out, grads = _run(m, batch, True, "bf16", bert_fp32=False)
    assert m.fused_body_calls == 1 and torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())
    _run(m, batch, False, "bf16", bert_fp32=False)
    assert m.fused_body_calls == 1                                        # the knob off: the stock call in either mode
