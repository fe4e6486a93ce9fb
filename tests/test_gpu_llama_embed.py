"""GPU checks of raw-text mode's Llama path: immtsf.ops.llama_embed_notes (csrc/llama_embed.hip + the GEMM family over the packed tokens)
against the float64 restatement tests/llama_embed_ref.py (pinned to transformers' padded call in tests/test_llama_embed_ref.py),
fusions.load_llm.embed_notes, the raw-text mode of TTF_T2V_XAttn / TTF_RecAvg and immtsf.text.embed_corpus.
Bodies, all 2 layers, head_dim 128, max_position_embeddings = max_length = 96:
  a: 2 heads over 1 K/V head (G = 2), 256 wide, intermediate 512, llama3 RoPE (original_max_position_embeddings 8: rescaled bands)
  b: 2 heads over 2 (G = 1), 256 wide, intermediate 512, default RoPE
  c: 4 heads over 1 (G = 4), 512 wide, intermediate 384, llama3 RoPE
Token counts 0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 96: the edges of the 32-key tile and of one and two 32-query tiles, where the causal
bound and the cut at a note's own length can go wrong; a second batch is a single 1-token note.  Ids are given directly, so the test
controls every count.
Bars, relative to the largest element: fp32 mode 1e-4; bf16 mode 4x the error, against float64, of transformers' own body
under torch.autocast(bfloat16) on the same inputs (measured per body and batch, printed)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_embed_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4
N_LAYER, N_POS, VOCAB = 2, 96, 50
BODIES = {"a": dict(n_head=2, n_kv=1, hidden=256, inner=512, rope=LR.LLAMA3_ROPE),
          "b": dict(n_head=2, n_kv=2, hidden=256, inner=512, rope=LR.DEFAULT_ROPE),
          "c": dict(n_head=4, n_kv=1, hidden=512, inner=384, rope=LR.LLAMA3_ROPE)}
BATCHES = {"edges": (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 96), "one_token": (1,)}
CASES = [(b, n) for b in BODIES for n in BATCHES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(body):
    return LR.build_llama(None, VOCAB, N_LAYER, max_pos=N_POS, head_dim=128, **BODIES[body]).requires_grad_(False).to(_dev())


@functools.lru_cache(maxsize=None)
def _notes(name):
    g = torch.Generator().manual_seed(23 + len(BATCHES[name]))
    return tuple(tuple(torch.randint(0, VOCAB, (n,), generator=g).tolist()) for n in BATCHES[name])


@functools.lru_cache(maxsize=None)
def _reference(body, name):
    """float64, computed once, shared"""
    m, b = _model(body), BODIES[body]
    return LR.embed_ragged(LR.weights64(m), [list(n) for n in _notes(name)], N_LAYER, b["n_head"], b["n_kv"], m.config.rms_norm_eps)


def _packed(notes, dev):
    ids = torch.tensor([t for n in notes for t in n], dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + list(torch.tensor([len(n) for n in notes]).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    return ids, cu


def _fused(body, name, precision):
    from immtsf import ops
    return ops.llama_embed_notes(_model(body), *_packed(_notes(name), _dev()), precision=precision)


def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("body,name", CASES)
def test_fp32_against_float64(body, name):
    out = _fused(body, name, "fp32")
    want = _reference(body, name)
    err = _rel(out, want)
    print(f"{body} {name}: fp32 {err:.2e} (bar {BAR:.0e})")
    assert out.shape == want.shape and out.dtype == torch.float32
    assert err < BAR


@functools.lru_cache(maxsize=None)
def _autocast_error(body, name):
    """the error, against float64, of transformers' own padded call under torch.autocast(bfloat16) + the masked mean in fp32"""
    dev = _dev()
    notes, want = _notes(name), _reference(body, name)
    ids = torch.zeros(len(notes), N_POS, dtype=torch.long)
    attn = torch.zeros(len(notes), N_POS, dtype=torch.long)
    for r, n in enumerate(notes):
        ids[r, :len(n)] = torch.tensor(n, dtype=torch.long)
        attn[r, :len(n)] = 1
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        hidden = _model(body)(input_ids=ids.to(dev), attention_mask=attn.to(dev)).last_hidden_state
    keep = attn.to(dev).unsqueeze(-1)
    hf = torch.where(keep > 0, hidden.float(), torch.zeros((), device=dev)).sum(1) / keep.sum(1).clamp(min=1)
    return _rel(hf, want)


@pytest.mark.parametrize("body,name", CASES)
def test_bf16_within_4x_of_autocast(body, name):
    ho = _autocast_error(body, name)
    eo = _rel(_fused(body, name, "bf16"), _reference(body, name))
    print(f"{body} {name}: bf16 {eo:.2e} (autocast {ho:.2e})")
    assert eo <= 4.0 * ho


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_zero_token_notes_are_exact_zero_rows_and_runs_repeat_bit_for_bit(precision):
    a, b = _fused("a", "edges", precision), _fused("a", "edges", precision)
    assert torch.equal(a, b)
    assert torch.equal(a[0], torch.zeros_like(a[0])) and torch.isfinite(a).all()
    from immtsf import ops
    dev = _dev()
    none = ops.llama_embed_notes(_model("a"), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev),
                                 precision=precision)
    assert none.shape == (2, 256) and not none.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_note_alone_and_inside_the_batch_agree(precision):
    """within the mode's bar (bit equality is not asked: the GEMM launcher may pick another kernel by row count)"""
    from immtsf import ops
    dev = _dev()
    notes, want = _notes("edges"), _reference("a", "edges")
    batch = _fused("a", "edges", precision)
    scale = float(want.abs().max())
    bar = BAR if precision == "fp32" else 4.0 * _autocast_error("a", "edges")
    for r in (1, 5, 10):
        alone = ops.llama_embed_notes(_model("a"), *_packed([notes[r]], dev), precision=precision)
        err = float((alone[0] - batch[r]).abs().max()) / scale
        print(f"{precision}: note {r} ({len(notes[r])} tokens) alone vs in the batch {err:.2e}")
        assert err < bar


def test_supported_limits():
    import note_embed_ref as NR

    from immtsf import ops
    dev = _dev()
    for body in BODIES:
        assert ops.llama_embed_notes_supported(_model(body), N_POS) and ops.llama_embed_notes_supported(_model(body), 1)
    assert not ops.llama_embed_notes_supported(_model("a"), N_POS + 1)                   # past max_position_embeddings
    assert not ops.llama_embed_notes_supported(torch.nn.Linear(4, 4), 8)

    def build(**kw):
        args = dict(n_head=2, n_kv=1, hidden=256, inner=512, head_dim=128, rope=LR.DEFAULT_ROPE)
        args.update(kw)
        return LR.build_llama(None, VOCAB, 1, max_pos=N_POS, **args).to(dev)

    assert ops.llama_embed_notes_supported(build(), 8)
    assert not ops.llama_embed_notes_supported(build(hidden=128, head_dim=64), 8)
    assert not ops.llama_embed_notes_supported(build(n_head=3, hidden=384), 8)            # G = 3
    assert not ops.llama_embed_notes_supported(build(hidden_act="gelu"), 8)
    assert not ops.llama_embed_notes_supported(build(rope={"rope_type": "dynamic", "rope_theta": 10000.0, "factor": 2.0}), 8)
    assert not ops.llama_embed_notes_supported(build().to(torch.bfloat16), 8)             # parameters stored in bf16
    assert not ops.llama_embed_notes_supported(build(attention_bias=True), 8)
    assert not ops.llama_embed_notes_supported(NR.build_model(None, VOCAB, 1, 128, 2, N_POS).to(dev), 8)          # a GPT2Model
    with pytest.raises(Exception):
        ops.llama_embed_notes(build(hidden=128, head_dim=64), *_packed([[1, 2, 3]], dev))


# ---- the front door: load_llm / embed_notes, the two TTF modules, the corpus helper --------------------------------------------------------
LETTERS = "abcdefghijklmnopqrstuvwxyz"
LONG = "river level rising after heavy rain, plan unchanged " * 3        # > 96 characters: truncated to 96 tokens
WINDOWS = [["seen at noon", "", LETTERS + " abcde", LONG], [], ["blood pressure stable overnight"]]
D = BODIES["a"]["hidden"]


@pytest.fixture()
def llm(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm, register_d_model
    LR.offline(monkeypatch)
    path = str(tmp_path / "llama")
    tok = LR.build_tokenizer(path)
    LR.build_llama(path, len(tok), N_LAYER, max_pos=N_POS, head_dim=128, attention_dropout=0.1, **BODIES["a"])
    register_d_model(path, D)
    tok, model = load_llm(path, N_LAYER, _dev())
    assert type(model).__name__ == "LlamaModel" and tok.pad_token == LR.EOS
    return path, tok, model


def _stock(notes, tok, model):
    from fusions import load_llm as L
    from immtsf import config
    was = config.note_embed_fused
    config.note_embed_fused = False
    try:
        before = dict(L.path_calls)
        with torch.no_grad():
            out = L.embed_notes(notes, tok, model, max_length=N_POS)
        assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]       # the knob
    finally:
        config.note_embed_fused = was
    return out


def test_embed_notes_takes_the_fused_path_and_matches_the_stock_one(llm):
    from fusions import load_llm as L
    _, tok, model = llm
    assert [len(tok(n).input_ids) for n in ("", "abc")] == [1, 4]
    before = dict(L.path_calls)
    out, mask = L.embed_notes(WINDOWS, tok, model, max_length=N_POS)
    assert L.path_calls["fused"] == before["fused"] + 1 and L.path_calls["stock"] == before["stock"]
    want, want_mask = _stock(WINDOWS, tok, model)
    assert out.shape == (3, 4, D) and out.is_cuda and mask.is_cuda and torch.equal(mask, want_mask)
    assert mask.tolist() == [[True] * 4, [False] * 4, [True, False, False, False]]
    err = _rel(out, want)              # over all B N_max rows: the padded-out notes are the begin-of-text token, not zero rows
    print(f"embed_notes fused vs stock on the GPU: {err:.2e}")
    assert err < BAR
    assert out[1, 0].any() and torch.equal(out[1, 0], out[2, 3]) and torch.equal(out[1, 0], out[0, 1])


def test_a_left_padding_tokenizer_takes_the_stock_path(llm):
    from fusions import load_llm as L
    _, _, model = llm
    tok = LR.build_tokenizer(None, padding_side="left")
    tok.pad_token = tok.eos_token
    before = dict(L.path_calls)
    with torch.no_grad():
        out, _ = L.embed_notes([["seen at noon", LETTERS]], tok, model, max_length=N_POS)
    assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]
    assert torch.isfinite(out).all()


def test_a_model_in_training_mode_with_dropout_takes_the_stock_path(llm):
    from fusions import load_llm as L
    _, tok, model = llm
    assert model.config.attention_dropout > 0
    before = dict(L.path_calls)
    try:
        with torch.no_grad():
            out, _ = L.embed_notes([["seen at noon", LETTERS]], tok, model.train(), max_length=N_POS)
    finally:
        model.eval()
    assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]
    assert torch.isfinite(out).all()


def test_a_token_id_past_the_table_raises_before_any_launch(llm):
    from fusions import load_llm as L
    _, tok, model = llm
    dev = _dev()
    ids = torch.zeros(3, N_POS, dtype=torch.long)
    attn = torch.zeros(3, N_POS, dtype=torch.long)
    ids[:, :3] = torch.tensor([0, 70, 71])
    attn[:, :3] = 1
    ids[1, 1] = len(tok)
    assert L._fused_ok(model, dev, N_POS, 3)           # (so the bad id never reaches a torch embedding lookup on the device)
    before = dict(L.path_calls)
    with pytest.raises(IndexError):
        L._pool_rows(model, ids, attn, torch.arange(3), dev)
    assert L.path_calls == before


@pytest.mark.parametrize("which", ["TTF_T2V_XAttn", "TTF_RecAvg"])
def test_raw_text_mode_equals_the_module_fed_the_stock_embeddings(llm, which):
    import importlib

    from immtsf.ops import PackedNotes
    path, tok, model = llm
    dev = _dev()
    cls = getattr(importlib.import_module(f"fusions.{which}"), which)
    extra = dict(n_heads_fusion=2) if which == "TTF_T2V_XAttn" else dict(recency_sigma=1.0)
    torch.manual_seed(3)
    raw = cls(path, N_LAYER, max_length=N_POS, device=str(dev), use_text_embeddings=False, dropout=0.1, d_txt=64, **extra).to(dev).eval()
    pre = cls(path, N_LAYER, max_length=N_POS, device=str(dev), use_text_embeddings=True, dropout=0.1, d_txt=64, **extra).to(dev).eval()
    pre.load_state_dict({k: v for k, v in raw.state_dict().items() if not k.startswith("llm_model.")})
    g = torch.Generator().manual_seed(4)
    tau = (torch.rand(3, 4, generator=g) * 24).to(dev)
    t_hat = torch.sort(torch.rand(3, 5, generator=g), 1).values.to(dev)
    from fusions import load_llm as L
    before = dict(L.path_calls)
    E, M = raw(WINDOWS, tau, t_hat)
    assert L.path_calls["fused"] > before["fused"] and L.path_calls["stock"] == before["stock"]
    V, mask = _stock(WINDOWS, tok, model)
    if which == "TTF_T2V_XAttn":       # the note mask is the lists': the precomputed path takes it as PackedNotes' lengths
        rows = V[mask]
        fed = PackedNotes(rows, torch.arange(rows.shape[0], dtype=torch.int32, device=dev), mask.sum(1).to(torch.int32), 4)
    else:
        fed = V
    E_want, _ = pre(fed, tau, t_hat)
    err = _rel(E, E_want)
    print(f"{which}: raw-text vs the stock path's embeddings E_txt {err:.2e}")
    assert E.shape == (3, 5, 64) and err < BAR
    assert M.dtype == torch.bool and M.view(-1).tolist() == [True, False, True]
    assert all(not p.requires_grad for p in raw.llm_model.parameters())


def test_embed_corpus_equals_embed_notes_note_by_note(llm):
    from fusions import load_llm as L
    from immtsf.text import embed_corpus
    _, tok, model = llm
    notes = [LETTERS, "seen at noon", "", LONG, "blood pressure stable", "a"]
    before = dict(L.path_calls)
    out = embed_corpus(notes, tok, model, max_length=N_POS, tokens_per_batch=96)
    assert L.path_calls["fused"] > before["fused"]
    assert out.shape == (6, D) and not out.is_cuda
    scale = float(out.abs().max())
    for i, note in enumerate(notes):
        one, _ = L.embed_notes([[note]], tok, model, max_length=N_POS)
        assert float((one[0, 0].cpu() - out[i]).abs().max()) / scale < BAR, i
