"""GPU checks of the fused frozen GPT-2 body (immtsf.ops.gpt2_body, csrc/gpt2.hip) against the float64 restatement tests/gpt2_ref.py
(pinned to transformers' GPT2Model in tests/test_gpt2_ref.py), and of its use in models/TimeLLM.py.
Bars: the project's fp32 bars, outputs 1e-4 and gradients 3e-4 relative to the largest element, in fp32 mode with and
without dropout; in bf16 mode 4x the error, against float64, of transformers' own body under torch.autocast(bfloat16) on the same
inputs (measured per shape, printed)."""
import functools
import math
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpt2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_BAR, GRAD_BAR = 1e-4, 3e-4
D, H = 128, 2
SHAPES = [(3, 37, 5), (2, 0, 9), (1, 1, 1), (2, 60, 4), (2, 17, 40), (1, 31, 65)]
CASES = [(s, 2) for s in SHAPES] + [((3, 37, 5), 1)]       # (B, S_p, S_t), n_layer
IDS = [f"B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for s, n in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _body(n_layer, p_drop, **kw):
    from transformers import GPT2Config, GPT2Model
    torch.manual_seed(11)
    cfg = GPT2Config(**{**dict(n_embd=D, n_head=H, n_layer=n_layer, n_positions=64, vocab_size=32, resid_pdrop=p_drop, embd_pdrop=p_drop,
                               attn_pdrop=p_drop), **dict(kw)})
    m = GPT2Model(cfg)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    for p in m.parameters():
        p.requires_grad = False
    return m.to(_dev()).train()


def _positions(shape):
    """the default body has 64 positions (test_supported_limits reads that bound); a longer sequence gets a body with a longer table"""
    return {"n_positions": 128} if shape[1] + shape[2] > 64 else {}


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    B, S_p, S_t = shape
    g = torch.Generator().manual_seed(100 + 7 * B + S_p + 3 * S_t)
    return tuple(torch.randn(B, n, D, generator=g) for n in (S_p, S_t, S_t))       # prefix, tail, upstream


@functools.lru_cache(maxsize=None)
def _reference(shape, n_layer):
    """float64, no dropout: computed once, shared"""
    prefix, tail, up = _inputs(shape)
    m = _body(n_layer, 0.0, **_positions(shape))
    return R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, H, m.config.layer_norm_epsilon)


def _rel(got, want):
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def _fused(m, shape, training=False, seed=None, prefix_grad=False):
    from immtsf import ops
    dev = _dev()
    prefix, tail, up = (t.to(dev) for t in _inputs(shape))
    tail = tail.clone().requires_grad_(True)
    prefix = prefix.clone().requires_grad_(prefix_grad)
    out = ops.gpt2_body(m, prefix, tail, training, seed=seed)
    (out * up).sum().backward()
    return out.detach(), tail.grad.detach(), prefix


@pytest.mark.parametrize("shape,n_layer", CASES, ids=IDS)
def test_fp32_against_float64(shape, n_layer):
    from immtsf import config
    config.precision = "fp32"
    out, grad, _ = _fused(_body(n_layer, 0.0, **_positions(shape)), shape)
    want_out, want_grad = _reference(shape, n_layer)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{shape} L{n_layer}: out {eo:.2e} (bar {OUT_BAR:.0e})  d tail {eg:.2e} (bar {GRAD_BAR:.0e})")
    assert out.shape == (shape[0], shape[2], D)
    assert eo < OUT_BAR and eg < GRAD_BAR


@pytest.mark.parametrize("shape,n_layer", CASES, ids=IDS)
def test_fp32_dropout_masks_reproduced(shape, n_layer):
    """all three dropouts at 0.3 in training mode: the masks rebuilt with ops.dropout_keep_mask feed the restatement; each kept fraction is
    within a binomial 5 sigma of 0.7"""
    from immtsf import config, ops
    config.precision = "fp32"
    dev = _dev()
    p, seed = 0.3, 0x5EED1234
    B, S_p, S_t = shape
    S = S_p + S_t
    m = _body(n_layer, p, **_positions(shape))
    out, grad, _ = _fused(m, shape, training=True, seed=seed)
    km = lambda site, n: ops.dropout_keep_mask(seed, site, n, p, dev).cpu()      # noqa: E731
    masks = {"p": (p, p, p), "embd": km(ops.GPT2_SITE_EMBD, B * S * D).view(B, S, D), "attn": [], "resid1": [], "resid2": []}
    for li in range(n_layer):
        sa, s1, s2 = ops.gpt2_sites(li)
        masks["attn"].append(km(sa, B * H * S * 1024).view(B, H, S, 1024)[..., :S])
        masks["resid1"].append(km(s1, B * S * D).view(B, S, D))
        masks["resid2"].append(km(s2, B * S * D).view(B, S, D))
    for name in ("embd", "attn", "resid1", "resid2"):
        for t in ([masks[name]] if name == "embd" else masks[name]):
            n = t.numel()
            frac = float(t.double().mean())
            assert abs(frac - 0.7) <= 5.0 * math.sqrt(0.7 * 0.3 / n), (name, frac, n)
    prefix, tail, up = _inputs(shape)
    want_out, want_grad = R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, H, m.config.layer_norm_epsilon, masks)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{shape} L{n_layer} dropout 0.3: out {eo:.2e}  d tail {eg:.2e}")
    assert eo < OUT_BAR and eg < GRAD_BAR


@pytest.mark.parametrize("shape,n_layer", CASES, ids=IDS)
def test_bf16_within_4x_of_autocast(shape, n_layer):
    from immtsf import config
    dev = _dev()
    m = _body(n_layer, 0.0, **_positions(shape))
    want_out, want_grad = _reference(shape, n_layer)
    prefix, tail, up = (t.to(dev) for t in _inputs(shape))
    t2 = tail.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        hf = m(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, -shape[2]:]
    (hf.float() * up).sum().backward()
    ho, hg = _rel(hf.float(), want_out), _rel(t2.grad, want_grad)
    config.precision = "bf16"
    out, grad, _ = _fused(m, shape)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{shape} L{n_layer} bf16: out {eo:.2e} (autocast {ho:.2e})  d tail {eg:.2e} (autocast {hg:.2e})")
    assert eo <= 4.0 * ho and eg <= 4.0 * hg


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
def test_two_runs_give_the_same_bits(p_drop):
    from immtsf import config
    config.precision = "fp32"
    m = _body(2, p_drop)
    a = _fused(m, (3, 37, 5), training=p_drop > 0, seed=77)
    b = _fused(m, (3, 37, 5), training=p_drop > 0, seed=77)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape,n_layer", CASES, ids=IDS)
def test_fused_equals_the_stock_body(shape, n_layer):
    """what models/TimeLLM.py computes with IMMTSF_TIMELLM_FUSED=0 -- transformers' GPT2Model over the concatenated rows, full autograd --
    on the same inputs: the attention kernel and the last-layer cut change nothing"""
    from immtsf import config
    config.precision = "fp32"
    dev = _dev()
    m = _body(n_layer, 0.0, **_positions(shape))
    prefix, tail, up = (t.to(dev) for t in _inputs(shape))
    t2 = tail.clone().requires_grad_(True)
    hf = m(inputs_embeds=torch.cat([prefix, t2], 1)).last_hidden_state[:, -shape[2]:]
    (hf * up).sum().backward()
    out, grad, _ = _fused(m, shape)
    eo = float((out - hf.detach()).abs().max() / hf.detach().abs().max())
    eg = float((grad - t2.grad).abs().max() / t2.grad.abs().max())
    print(f"{shape} L{n_layer}: fused vs stock out {eo:.2e}  d tail {eg:.2e}")
    assert eo < OUT_BAR and eg < GRAD_BAR


def test_prefix_may_require_grad_and_gets_none():
    from immtsf import config
    config.precision = "fp32"
    _, grad, prefix = _fused(_body(2, 0.0), (3, 37, 5), prefix_grad=True)
    assert prefix.requires_grad and prefix.grad is None and torch.isfinite(grad).all()


def test_no_grad_saves_nothing():
    from immtsf import ops
    dev = _dev()
    prefix, tail, _ = (t.to(dev) for t in _inputs((3, 37, 5)))
    with torch.no_grad():
        out = ops.gpt2_body(_body(2, 0.0), prefix, tail.clone().requires_grad_(True), False)
    assert out.grad_fn is None and not out.requires_grad


def test_supported_limits():
    from immtsf import ops
    assert ops.gpt2_body_supported(_body(2, 0.0), 37, 5)
    assert ops.gpt2_body_supported(_body(2, 0.0), 60, 4)
    assert not ops.gpt2_body_supported(_body(2, 0.0), 60, 5)                               # S > n_positions
    assert not ops.gpt2_body_supported(_body(2, 0.0, n_head=4), 37, 5)                     # head_dim 32
    assert not ops.gpt2_body_supported(_body(2, 0.0, activation_function="gelu"), 37, 5)
    assert not ops.gpt2_body_supported(torch.nn.Linear(4, 4), 37, 5)


def _timellm(dev):
    from models.TimeLLM import TimeLLM
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="GPT2", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device=str(dev),
                                immtsf_offline_llm=dict(vocab_size=320, n_positions=512))          # body dropouts at GPT2Config's 0.1
    torch.manual_seed(0)
    m = TimeLLM(cfg).to(dev).train()
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    g = torch.Generator().manual_seed(1)
    data = torch.randn(3, 12, 3, generator=g).to(dev)
    mask = (torch.rand(3, 12, 3, generator=g) < 0.8).float().to(dev)
    tp = torch.sort(torch.rand(3, 12, generator=g), 1).values.to(dev)
    return m, (torch.rand(3, 5, generator=g).to(dev), data * mask, tp, mask)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "knob_off"])
def test_timellm_takes_the_fused_body(fused):
    from immtsf import config
    dev = _dev()
    was = config.timellm_fused
    config.timellm_fused = fused
    try:
        m, batch = _timellm(dev)
        assert m.llm_model.training and m.llm_model.config.resid_pdrop == 0.1
        out = m.forecasting(*batch)
        out.square().mean().backward()
    finally:
        config.timellm_fused = was
    assert out.shape == (3, 5, 3) and torch.isfinite(out).all()
    assert m.fused_body_calls == (1 if fused else 0)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        else:
            assert p.grad is None, k
