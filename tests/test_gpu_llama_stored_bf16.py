"""GPU checks of a frozen Llama STORED in bf16 on immtsf.ops.llama_embed_notes / llama_body (immtsf.config.llama_stored_bf16):
the weights are read in place -- fp32 mode on immtsf_gemm_asplit, bf16 mode with the parameter's storage as the GEMM family's bf16 image,
the row kernels through their _p16 entry points, q | k | v and gate | up as products side by side -- and no second image of any weight is
made.  Models are built as from_pretrained leaves a bf16 checkpoint: built in fp32, then every parameter's data cast to bf16, buffers
(rotary_emb.inv_freq) untouched.  The truth is the float64 restatement (tests/llama_embed_ref.py, llama_body_ref.py) on the bf16 VALUES.
Bodies a, b, c, note batches and body shapes: those of tests/test_gpu_llama_embed.py / test_gpu_llama_body.py (2 layers, head_dim 128,
max_position_embeddings 96).
Bars, relative to the largest element: fp32 mode 1e-4 for the pooled rows and the body's output, 3e-4 for d tail; bf16 mode
4x the error, against float64, of transformers' own call under torch.autocast(bfloat16) on an fp32 up-cast copy of the same model (the same
weight values), measured per case.  The error of the stock call on the bf16 model itself is printed beside them, not asserted."""
import copy
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_body_ref as R  # noqa: E402
import llama_embed_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
BAR, GRAD_BAR = 1e-4, 3e-4
N_POS, VOCAB = 96, 50
BODIES = {"a": dict(n_head=2, n_kv=1, hidden=256, inner=512, rope=LR.LLAMA3_ROPE),
          "b": dict(n_head=2, n_kv=2, hidden=256, inner=512, rope=LR.DEFAULT_ROPE),
          "c": dict(n_head=4, n_kv=1, hidden=512, inner=384, rope=LR.LLAMA3_ROPE)}
BATCHES = {"edges": (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 96), "one_token": (1,)}
NOTE_CASES = [(b, n) for b in BODIES for n in BATCHES]
SHAPE_CASES = [((3, 37, 5), 2), ((2, 0, 33), 2), ((1, 1, 1), 2), ((2, 17, 40), 2), ((1, 31, 65), 2), ((3, 37, 5), 1)]      # (B, S_p, S_t), layers
BODY_CASES = [(b, s, n) for b in BODIES for s, n in SHAPE_CASES]
BODY_IDS = [f"{b}_B{s[0]}_Sp{s[1]}_St{s[2]}_L{n}" for b, s, n in BODY_CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture()
def knob(monkeypatch):
    import immtsf
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", True)


def _store_bf16(m):
    """what from_pretrained leaves of a bf16 checkpoint: every parameter bf16, the buffers as they were"""
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m


def _build(n_layer=2, body="a", **kw):
    args = dict(BODIES[body], head_dim=128)
    args.update(kw)
    return LR.build_llama(None, VOCAB, n_layer, max_pos=N_POS, **args).requires_grad_(False)


@functools.lru_cache(maxsize=None)
def _stored(body, n_layer=2):
    return _store_bf16(_build(n_layer, body)).to(_dev())


@functools.lru_cache(maxsize=None)
def _upcast(body, n_layer=2):
    """an fp32 model with the stored model's weight values"""
    m = _store_bf16(_build(n_layer, body))
    for p in m.parameters():
        p.data = p.data.float()
    return m.to(_dev())


def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def _packed(notes, dev):
    ids = torch.tensor([t for n in notes for t in n], dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + list(torch.tensor([len(n) for n in notes]).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    return ids, cu


def _frozen_tensors(model):
    found = []

    def walk(o):
        if torch.is_tensor(o):
            found.append(o)
        elif isinstance(o, (tuple, list)):
            for x in o:
                walk(x)
        elif isinstance(o, dict):
            for x in o.values():
                walk(x)
        elif hasattr(o, "__slots__"):
            for s in o.__slots__:
                walk(getattr(o, s, None))
    walk(model.__dict__.get("_immtsf_frozen", {}))
    return found


def _storage_state(model):
    return [(p.data_ptr(), p._version, p.dtype) for p in model.parameters()]


# ---- raw-text mode: llama_embed_notes ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _notes(name):
    g = torch.Generator().manual_seed(23 + len(BATCHES[name]))
    return tuple(tuple(torch.randint(0, VOCAB, (n,), generator=g).tolist()) for n in BATCHES[name])


@functools.lru_cache(maxsize=None)
def _note_reference(body, name):
    m, b = _stored(body), BODIES[body]
    return LR.embed_ragged(LR.weights64(m), [list(n) for n in _notes(name)], 2, b["n_head"], b["n_kv"], m.config.rms_norm_eps)


def _embed(model, name, precision):
    from immtsf import ops
    return ops.llama_embed_notes(model, *_packed(_notes(name), _dev()), precision=precision)


def _padded_pool(model, name, autocast):
    """transformers' padded call on `model` + the masked mean in fp32"""
    dev = _dev()
    notes = _notes(name)
    ids = torch.zeros(len(notes), N_POS, dtype=torch.long)
    attn = torch.zeros(len(notes), N_POS, dtype=torch.long)
    for r, n in enumerate(notes):
        ids[r, :len(n)] = torch.tensor(n, dtype=torch.long)
        attn[r, :len(n)] = 1
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        hidden = model(input_ids=ids.to(dev), attention_mask=attn.to(dev)).last_hidden_state
    keep = attn.to(dev).unsqueeze(-1)
    return torch.where(keep > 0, hidden.float(), torch.zeros((), device=dev)).sum(1) / keep.sum(1).clamp(min=1)


@functools.lru_cache(maxsize=None)
def _note_autocast_error(body, name):
    return _rel(_padded_pool(_upcast(body), name, True), _note_reference(body, name))


@pytest.mark.parametrize("body,name", NOTE_CASES)
def test_notes_fp32_mode_against_float64(knob, body, name):
    from immtsf import ops
    m = _stored(body)
    before, state = ops.asplit_product_calls, _storage_state(m)
    out = _embed(m, name, "fp32")
    want = _note_reference(body, name)
    err = _rel(out, want)
    print(f"{body} {name}: stored bf16, fp32 mode {err:.2e} (bar {BAR:.0e})")
    assert out.shape == want.shape and out.dtype == torch.float32
    assert err < BAR
    assert ops.asplit_product_calls >= before + 2 * 7          # q, k, v, o, gate, up, down of both layers
    assert not _frozen_tensors(m) and _storage_state(m) == state


@pytest.mark.parametrize("body,name", NOTE_CASES)
def test_notes_bf16_mode_within_4x_of_autocast(knob, body, name):
    m = _stored(body)
    state = _storage_state(m)
    want = _note_reference(body, name)
    ho = _note_autocast_error(body, name)
    so = _rel(_padded_pool(m, name, False), want)
    eo = _rel(_embed(m, name, "bf16"), want)
    print(f"{body} {name}: stored bf16, bf16 mode {eo:.2e} (autocast on the up-cast copy {ho:.2e}; stock call on the bf16 model {so:.2e})")
    assert eo <= 4.0 * ho
    assert not _frozen_tensors(m) and _storage_state(m) == state


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_notes_repeat_bit_for_bit_and_a_zero_token_note_is_an_exact_zero_row(knob, precision):
    a, b = _embed(_stored("a"), "edges", precision), _embed(_stored("a"), "edges", precision)
    assert torch.equal(a, b)
    assert torch.equal(a[0], torch.zeros_like(a[0])) and bool(a[1:].any()) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_model_made_with_to_bfloat16_reads_its_own_rounded_inv_freq(knob, precision):
    """.to(torch.bfloat16) rounds the rotary buffer too; the operator and the restatement both read that buffer as it stands"""
    from immtsf import ops
    b = BODIES["a"]
    m = _build(2, "a").to(torch.bfloat16).to(_dev())
    assert m.rotary_emb.inv_freq.dtype == torch.bfloat16 and ops.llama_embed_notes_supported(m, N_POS)
    want = LR.embed_ragged(LR.weights64(m), [list(n) for n in _notes("edges")], 2, b["n_head"], b["n_kv"], m.config.rms_norm_eps)
    err = _rel(_embed(m, "edges", precision), want)
    if precision == "fp32":
        bar = BAR
    else:           # the autocast call of an fp32 up-cast copy of THIS model: .float() keeps the rounded buffer's values
        bar = 4.0 * _rel(_padded_pool(copy.deepcopy(m).float(), "edges", True), want)
    print(f".to(bfloat16) model, {precision} mode: {err:.2e} (bar {bar:.2e})")
    assert err <= bar


def test_knob_and_support_limits(monkeypatch):
    import immtsf
    from immtsf import ops
    dev = _dev()
    m = _stored("a")
    ids, cu = _packed([[1, 2, 3]], dev)
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", False)
    assert not ops.llama_embed_notes_supported(m, 8) and not ops.llama_body_supported(m, 3, 5)
    with pytest.raises(Exception):
        ops.llama_embed_notes(m, ids, cu)
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", True)
    assert ops.llama_embed_notes_supported(m, 8) and ops.llama_embed_notes_supported(m, N_POS) and ops.llama_body_supported(m, 3, 5)
    assert not ops.llama_embed_notes_supported(m, N_POS + 1) and not ops.llama_body_supported(m, 92, 5)
    mixed = _store_bf16(_build(1)).to(dev)
    mixed.norm.weight.data = mixed.norm.weight.data.float()
    bad = [mixed, _build(1).to(torch.float16).to(dev), _store_bf16(_build(1, hidden=128, head_dim=64)).to(dev),
           _store_bf16(_build(1, rope={"rope_type": "dynamic", "rope_theta": 10000.0, "factor": 2.0})).to(dev)]
    for x in bad:
        assert not ops.llama_embed_notes_supported(x, 8) and not ops.llama_body_supported(x, 3, 5)
    assert ops.llama_embed_notes_supported(_store_bf16(_build(1)).to(dev), 8)
    assert ops.llama_embed_notes_supported(_upcast("a"), 8)          # an fp32 model is what it was, knob on or off


# ---- TimeLLM's body: llama_body ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape, d):
    B, S_p, S_t = shape
    g = torch.Generator().manual_seed(100 + 7 * B + S_p + 3 * S_t)
    return tuple(torch.randn(B, n, d, generator=g) for n in (S_p, S_t, S_t))       # prefix, tail, upstream


@functools.lru_cache(maxsize=None)
def _body_reference(body, shape, n_layer):
    m, b = _stored(body, n_layer), BODIES[body]
    prefix, tail, up = _inputs(shape, b["hidden"])
    return R.tail_forward_backward(R.weights64(m), prefix, tail, up, n_layer, b["n_head"], b["n_kv"], m.config.rms_norm_eps)


def _body(body, shape, n_layer, precision):
    from immtsf import ops
    dev = _dev()
    prefix, tail, up = (t.to(dev) for t in _inputs(shape, BODIES[body]["hidden"]))
    tail = tail.clone().requires_grad_(True)
    out = ops.llama_body(_stored(body, n_layer), prefix, tail, False, precision=precision)
    (out * up).sum().backward()
    return out.detach(), tail.grad.detach()


def _stock_body(model, shape, d, autocast, dtype=torch.float32):
    dev = _dev()
    prefix, tail, up = (t.to(dev) for t in _inputs(shape, d))
    t2 = tail.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        hf = model(inputs_embeds=torch.cat([prefix, t2], 1).to(dtype)).last_hidden_state[:, -shape[2]:]
    (hf.float() * up).sum().backward()
    return hf.float().detach(), t2.grad.detach()


@pytest.mark.parametrize("body,shape,n_layer", BODY_CASES, ids=BODY_IDS)
def test_body_fp32_mode_against_float64(knob, body, shape, n_layer):
    from immtsf import ops
    m = _stored(body, n_layer)
    before, state = ops.asplit_product_calls, _storage_state(m)
    out, grad = _body(body, shape, n_layer, "fp32")
    want_out, want_grad = _body_reference(body, shape, n_layer)
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{body} {shape} L{n_layer}: stored bf16, fp32 mode out {eo:.2e} (bar {BAR:.0e})  d tail {eg:.2e} (bar {GRAD_BAR:.0e})")
    assert out.shape == (shape[0], shape[2], BODIES[body]["hidden"]) and out.dtype == torch.float32 and grad.dtype == torch.float32
    assert eo < BAR and eg < GRAD_BAR
    assert ops.asplit_product_calls >= before + 14 * n_layer          # seven products forward, seven backward, a layer
    assert not _frozen_tensors(m) and _storage_state(m) == state


@pytest.mark.parametrize("body,shape,n_layer", BODY_CASES, ids=BODY_IDS)
def test_body_bf16_mode_within_4x_of_autocast(knob, body, shape, n_layer):
    m, d = _stored(body, n_layer), BODIES[body]["hidden"]
    state = _storage_state(m)
    want_out, want_grad = _body_reference(body, shape, n_layer)
    hf, hg = _stock_body(_upcast(body, n_layer), shape, d, True)
    ho, hgr = _rel(hf, want_out), _rel(hg, want_grad)
    sf, sg = _stock_body(m, shape, d, False, torch.bfloat16)
    out, grad = _body(body, shape, n_layer, "bf16")
    eo, eg = _rel(out, want_out), _rel(grad, want_grad)
    print(f"{body} {shape} L{n_layer}: stored bf16, bf16 mode out {eo:.2e} (autocast on the up-cast copy {ho:.2e}; stock call on the bf16 "
          f"model {_rel(sf, want_out):.2e})  d tail {eg:.2e} (autocast {hgr:.2e}; stock {_rel(sg, want_grad):.2e})")
    assert eo <= 4.0 * ho and eg <= 4.0 * hgr
    assert not _frozen_tensors(m) and _storage_state(m) == state


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_body_repeats_bit_for_bit(knob, precision):
    for body, shape in (("a", (2, 17, 40)), ("c", (3, 37, 5))):
        a, b = _body(body, shape, 2, precision), _body(body, shape, 2, precision)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the front doors ----------------------------------------------------------------------------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
LONG = "river level rising after heavy rain, plan unchanged " * 3        # > 96 characters: truncated to 96 tokens
WINDOWS = [["seen at noon", "", LETTERS + " abcde", LONG], [], ["blood pressure stable overnight"]]
D = BODIES["a"]["hidden"]


@pytest.fixture()
def llm(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm, register_d_model
    LR.offline(monkeypatch)
    path = str(tmp_path / "llama_bf16")
    tok = LR.build_tokenizer(path)
    LR.build_llama(None, len(tok), 2, max_pos=N_POS, head_dim=128, **BODIES["a"]).to(torch.bfloat16).save_pretrained(path)
    register_d_model(path, D)
    tok, model = load_llm(path, 2, _dev())
    assert type(model).__name__ == "LlamaModel" and all(p.dtype == torch.bfloat16 and p.is_cuda for p in model.parameters())
    assert model.rotary_emb.inv_freq.dtype == torch.float32
    return tok, model


def _embed_notes_by(route, tok, model, monkeypatch):
    import immtsf
    from fusions import load_llm as L
    monkeypatch.setattr(immtsf.config, "llama_stored_bf16", route == "fused")
    before = dict(L.path_calls)
    with torch.no_grad():
        out = L.embed_notes(WINDOWS, tok, model, max_length=N_POS)
    other = "stock" if route == "fused" else "fused"
    assert L.path_calls[route] == before[route] + 1 and L.path_calls[other] == before[other]
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_load_llm_returns_a_stored_bf16_model_and_embed_notes_takes_the_fused_path(llm, monkeypatch, precision):
    import immtsf
    tok, model = llm
    monkeypatch.setattr(immtsf.config, "precision", precision)
    want, want_mask = _embed_notes_by("stock", tok, model, monkeypatch)          # knob off: the padded call
    out, mask = _embed_notes_by("fused", tok, model, monkeypatch)
    assert out.dtype == torch.bfloat16 and want.dtype == torch.bfloat16 and out.shape == want.shape == (3, 4, D)
    assert torch.equal(mask, want_mask) and mask.tolist() == [[True] * 4, [False] * 4, [True, False, False, False]]
    # the stock call's own error against float64, over the rows the windows hold (a padded-out note is the empty string: the BOS token alone)
    flat = [n for w in WINDOWS for n in list(w) + [""] * (4 - len(w))]
    ids = [tok(n, truncation=True, max_length=N_POS).input_ids for n in flat]
    b = BODIES["a"]
    ref = LR.embed_ragged(LR.weights64(model), ids, 2, b["n_head"], b["n_kv"], model.config.rms_norm_eps).view(3, 4, D)
    stock_err, err = _rel(want, ref), _rel(out, want)
    print(f"embed_notes on a stored-bf16 model, {precision} mode: fused vs stock {err:.2e}; stock vs float64 {stock_err:.2e}; "
          f"fused vs float64 {_rel(out, ref):.2e}")
    assert err <= 4.0 * stock_err
    assert not _frozen_tensors(model)


def _timellm(dev):
    from models.TimeLLM import TimeLLM
    stand_in = dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, intermediate_size=512, vocab_size=320)
    cfg = types.SimpleNamespace(input_len=16, pred_len=8, use_norm=True, d_ff=32, ts_vocab_size=20, input_token_len=8, stride=4,
                                domain_des="synthetic", top_k=3, C=3, llm_model_timellm="LLAMA", llm_layers_timellm=2, dropout=0.0,
                                d_model=16, n_heads=2, batch_size=4, device=str(dev), immtsf_offline_llm=stand_in)
    torch.manual_seed(0)
    m = TimeLLM(cfg).to(dev).train()
    _store_bf16(m.llm_model)
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
        config.manual_seed(7)
        m.zero_grad(set_to_none=True)
        out = m.forecasting(*batch)
        out.square().mean().backward()
    finally:
        config.timellm_fused, config.precision = was, was_p
    return out.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.requires_grad}


def test_timellm_runs_a_stored_bf16_body_on_the_fused_route(knob):
    """fp32 mode: within the body bars of the same module with the body up-cast to fp32, run on transformers' stock call"""
    dev = _dev()
    m, batch = _timellm(dev)
    assert all(p.dtype == torch.bfloat16 for p in m.llm_model.parameters()) and not any(p.requires_grad for p in m.llm_model.parameters())
    out, grads = _run(m, batch, True)
    assert m.fused_body_calls == 1
    assert out.shape == (3, 5, 3) and bool(torch.isfinite(out).all()) and len(grads) > 0
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert not _frozen_tensors(m.llm_model)
    for p in m.llm_model.parameters():
        p.data = p.data.float()
    want, want_grads = _run(m, batch, False)
    assert m.fused_body_calls == 1
    eo = _rel(out, want)
    print(f"TimeLLM, stored-bf16 Llama stand-in, fused vs the up-cast body's stock call: out {eo:.2e}")
    assert eo < BAR
    assert set(grads) == set(want_grads)
    scale = {}          # per layer (weight and bias together), as tests/test_gpu_llama_body.py takes it
    for k, g in want_grads.items():
        owner = k.rsplit(".", 1)[0]
        scale[owner] = max(scale.get(owner, 0.0), float(g.abs().max()))
    for k in grads:
        eg = float((grads[k] - want_grads[k]).abs().max()) / scale[k.rsplit(".", 1)[0]]
        print(f"  d {k}: {eg:.2e}")
        assert eg < GRAD_BAR, k
