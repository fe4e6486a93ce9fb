"""GPU checks of raw-text mode's BERT path: immtsf.ops.bert_embed_notes (csrc/bert_embed.hip + the non-causal ragged attention of
csrc/note_embed.hip + the GEMM family over the packed tokens) against the float64 restatement tests/bert_embed_ref.py (pinned to
transformers' padded call in tests/test_bert_embed_ref.py), fusions.load_llm.embed_notes, the raw-text mode of TTF_T2V_XAttn / TTF_RecAvg
and immtsf.text.embed_corpus.
Body: 2 layers, 128 wide, 2 heads, intermediate 512, max_position_embeddings = max_length = 96.  Token counts 0, 1, 2, 31, 32, 33, 63, 64,
65, 96, 96: the edges of a 32-key tile and a 64-query wave, where the masking of a note's tail by its own length can go wrong; a second
batch is a single 1-token note.  Ids are given directly, so the test controls every count.
Bars, relative to the largest element: fp32 mode 1e-4; bf16 mode 4x the error, against float64, of transformers' own body
under torch.autocast(bfloat16) on the same inputs (measured per batch, printed)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_embed_ref as BR  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4
N_LAYER, D, H, INNER, N_POS, VOCAB = 2, 128, 2, 512, 96, 50
BATCHES = {"edges": (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 96), "one_token": (1,)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model():
    return BR.build_bert(None, VOCAB, N_LAYER, D, H, INNER, N_POS).requires_grad_(False).to(_dev())


@functools.lru_cache(maxsize=None)
def _notes(name):
    g = torch.Generator().manual_seed(23 + len(BATCHES[name]))
    return tuple(tuple(torch.randint(0, VOCAB, (n,), generator=g).tolist()) for n in BATCHES[name])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64, computed once, shared"""
    m = _model()
    return BR.embed_ragged(BR.weights64(m), [list(n) for n in _notes(name)], N_LAYER, H, m.config.layer_norm_eps)


def _packed(notes, dev):
    ids = torch.tensor([t for n in notes for t in n], dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + list(torch.tensor([len(n) for n in notes]).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    return ids, cu


def _fused(name, precision):
    from immtsf import ops
    return ops.bert_embed_notes(_model(), *_packed(_notes(name), _dev()), precision=precision)


def _rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("name", list(BATCHES))
def test_fp32_against_float64(name):
    out = _fused(name, "fp32")
    want = _reference(name)
    err = _rel(out, want)
    print(f"{name}: fp32 {err:.2e} (bar {BAR:.0e})")
    assert out.shape == want.shape and out.dtype == torch.float32
    assert err < BAR


@functools.lru_cache(maxsize=None)
def _autocast_error(name):
    """the error, against float64, of transformers' own padded call under torch.autocast(bfloat16) + the masked mean in fp32"""
    dev = _dev()
    notes, want = _notes(name), _reference(name)
    ids = torch.zeros(len(notes), N_POS, dtype=torch.long)
    attn = torch.zeros(len(notes), N_POS, dtype=torch.long)
    for r, n in enumerate(notes):
        ids[r, :len(n)] = torch.tensor(n, dtype=torch.long)
        attn[r, :len(n)] = 1
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        hidden = _model()(input_ids=ids.to(dev), attention_mask=attn.to(dev)).last_hidden_state
    keep = attn.to(dev).unsqueeze(-1)
    hf = torch.where(keep > 0, hidden.float(), torch.zeros((), device=dev)).sum(1) / keep.sum(1).clamp(min=1)
    return _rel(hf, want)


@pytest.mark.parametrize("name", list(BATCHES))
def test_bf16_within_4x_of_autocast(name):
    ho = _autocast_error(name)
    eo = _rel(_fused(name, "bf16"), _reference(name))
    print(f"{name}: bf16 {eo:.2e} (autocast {ho:.2e})")
    assert eo <= 4.0 * ho


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_zero_token_notes_are_exact_zero_rows_and_runs_repeat_bit_for_bit(precision):
    a, b = _fused("edges", precision), _fused("edges", precision)
    assert torch.equal(a, b)
    assert torch.equal(a[0], torch.zeros_like(a[0])) and torch.isfinite(a).all()
    from immtsf import ops
    dev = _dev()
    none = ops.bert_embed_notes(_model(), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev),
                                precision=precision)
    assert none.shape == (2, D) and not none.any()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_note_alone_and_inside_the_batch_agree(precision):
    """within the mode's bar (bit equality is not asked: the GEMM launcher may pick another kernel by row count)"""
    from immtsf import ops
    dev = _dev()
    notes, want = _notes("edges"), _reference("edges")
    batch = _fused("edges", precision)
    scale = float(want.abs().max())
    bar = BAR if precision == "fp32" else 4.0 * _autocast_error("edges")
    for r in (1, 5, 10):
        alone = ops.bert_embed_notes(_model(), *_packed([notes[r]], dev), precision=precision)
        err = float((alone[0] - batch[r]).abs().max()) / scale
        print(f"{precision}: note {r} ({len(notes[r])} tokens) alone vs in the batch {err:.2e}")
        assert err < bar


def test_supported_limits():
    import note_embed_ref as NR

    from immtsf import ops
    m, dev = _model(), _dev()
    assert ops.bert_embed_notes_supported(m, N_POS) and ops.bert_embed_notes_supported(m, 1)
    assert not ops.bert_embed_notes_supported(m, N_POS + 1)                     # past max_position_embeddings
    assert not ops.bert_embed_notes_supported(torch.nn.Linear(4, 4), 8)
    assert not ops.bert_embed_notes_supported(BR.build_bert(None, VOCAB, 1, 128, 4, INNER, N_POS).to(dev), 8)        # head_dim 32
    assert not ops.bert_embed_notes_supported(BR.build_bert(None, VOCAB, 1, D, H, INNER, N_POS, hidden_act="relu").to(dev), 8)
    assert not ops.bert_embed_notes_supported(NR.build_model(None, VOCAB, 1, D, H, N_POS).to(dev), 8)                # a GPT2Model


# ---- the front door: load_llm / embed_notes, the two TTF modules, the corpus helper --------------------------------------------------------
LETTERS = "a b c d e f g h i j k l m n o p q r s t u v w x y z"
LONG = "river level rising after heavy rain , plan unchanged " * 3        # > 96 characters: truncated to 96 tokens
WINDOWS = [["seen at noon", "", LETTERS + " a b c d e", LONG], [], ["blood pressure stable overnight"]]


@pytest.fixture()
def llm(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm, register_d_model
    BR.offline(monkeypatch)
    path = str(tmp_path / "bert")
    tok, _ = BR.build_local_bert(path, N_LAYER, D, H, INNER, N_POS)
    assert len(tok) == VOCAB
    register_d_model(path, D)
    tok, model = load_llm(path, N_LAYER, _dev())
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
    assert [len(tok(n).input_ids) for n in ("", "a b c")] == [2, 5]
    before = dict(L.path_calls)
    out, mask = L.embed_notes(WINDOWS, tok, model, max_length=N_POS)
    assert L.path_calls["fused"] == before["fused"] + 1 and L.path_calls["stock"] == before["stock"]
    want, want_mask = _stock(WINDOWS, tok, model)
    assert out.shape == (3, 4, D) and out.is_cuda and mask.is_cuda and torch.equal(mask, want_mask)
    assert mask.tolist() == [[True] * 4, [False] * 4, [True, False, False, False]]
    err = _rel(out, want)              # over all B N_max rows: the padded-out notes are [CLS] [SEP], not zero rows
    print(f"embed_notes fused vs stock on the GPU: {err:.2e}")
    assert err < BAR
    assert out[1, 0].any() and torch.equal(out[1, 0], out[2, 3]) and torch.equal(out[1, 0], out[0, 1])


def test_a_left_padding_tokenizer_takes_the_stock_path(llm):
    from fusions import load_llm as L
    _, _, model = llm
    tok = BR.build_wordpiece_tokenizer(None, padding_side="left")
    before = dict(L.path_calls)
    with torch.no_grad():
        out, _ = L.embed_notes([["seen at noon", LETTERS]], tok, model, max_length=N_POS)
    assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]
    assert torch.isfinite(out).all()


def test_a_model_in_training_mode_with_dropout_takes_the_stock_path(llm):
    from fusions import load_llm as L
    _, tok, model = llm
    assert model.config.hidden_dropout_prob > 0
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
    _, _, model = llm
    dev = _dev()
    ids = torch.zeros(3, N_POS, dtype=torch.long)
    attn = torch.zeros(3, N_POS, dtype=torch.long)
    ids[:, :3] = torch.tensor([2, 7, 3])
    attn[:, :3] = 1
    ids[1, 1] = VOCAB
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
