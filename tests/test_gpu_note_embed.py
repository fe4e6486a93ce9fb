"""GPU checks of raw-text mode: immtsf.ops.gpt2_embed_notes (csrc/note_embed.hip + the GEMM family + the row kernels of csrc/gpt2.hip over
the packed tokens) against the float64 restatement tests/note_embed_ref.py (pinned to transformers' padded call in
tests/test_note_embed_ref.py), fusions.load_llm.embed_notes, the raw-text mode of TTF_T2V_XAttn / TTF_RecAvg and immtsf.text.embed_corpus.
Body: 2 layers, 128 wide, 2 heads, n_positions = max_length = 96.  Token counts 0, 1, 31, 32, 33, 63, 64, 65, 96 and a second 96 (the
note the tokenizer truncates): the edges of a 32-key tile and a 64-query wave; a second batch is a single 1-token note.
Bars, relative to the largest element: fp32 mode 1e-4; bf16 mode 4x the error, against float64, of transformers' own body
under torch.autocast(bfloat16) on the same inputs (measured per batch, printed)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_embed_ref as NR  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4
N_LAYER, D, H, N_POS, VOCAB = 2, 128, 2, 96, 257
BATCHES = {"edges": (0, 1, 31, 32, 33, 63, 64, 65, 96, 96), "one_token": (1,)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model():
    return NR.build_model(None, VOCAB, N_LAYER, D, H, N_POS).requires_grad_(False).to(_dev())


@functools.lru_cache(maxsize=None)
def _notes(name):
    g = torch.Generator().manual_seed(17 + len(BATCHES[name]))
    return tuple(tuple(torch.randint(0, VOCAB, (n,), generator=g).tolist()) for n in BATCHES[name])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64, computed once, shared"""
    m = _model()
    return NR.embed_ragged(NR.weights64(m), [list(n) for n in _notes(name)], N_LAYER, H, m.config.layer_norm_epsilon)


def _packed(notes, dev):
    ids = torch.tensor([t for n in notes for t in n], dtype=torch.int32, device=dev)
    cu = torch.tensor([0] + list(torch.tensor([len(n) for n in notes]).cumsum(0).tolist()), dtype=torch.int32, device=dev)
    return ids, cu


def _fused(name, precision):
    from immtsf import ops
    return ops.gpt2_embed_notes(_model(), *_packed(_notes(name), _dev()), precision=precision)


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
    hf = (hidden.float() * keep).sum(1) / keep.sum(1).clamp(min=1)
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
    none = ops.gpt2_embed_notes(_model(), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev),
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
    for r in (1, 4, 9):
        alone = ops.gpt2_embed_notes(_model(), *_packed([notes[r]], dev), precision=precision)
        err = float((alone[0] - batch[r]).abs().max()) / scale
        print(f"{precision}: note {r} ({len(notes[r])} tokens) alone vs in the batch {err:.2e}")
        assert err < bar


def test_supported_limits():
    from immtsf import ops
    m = _model()
    assert ops.gpt2_embed_notes_supported(m, N_POS) and ops.gpt2_embed_notes_supported(m, 1)
    assert not ops.gpt2_embed_notes_supported(m, N_POS + 1)                     # past n_positions
    assert not ops.gpt2_embed_notes_supported(torch.nn.Linear(4, 4), 8)
    assert not ops.gpt2_embed_notes_supported(NR.build_model(None, VOCAB, 1, 128, 4, N_POS).to(_dev()), 8)      # head_dim 32


# ---- the front door: load_llm / embed_notes, the two TTF modules, the corpus helper --------------------------------------------------------
LONG = "river level rising after heavy rain, plan unchanged; " * 3        # > 96 characters: truncated to 96 tokens
WINDOWS = [["seen at noon", "", "x" * 33, LONG], [], ["blood pressure stable overnight"]]


@pytest.fixture()
def llm(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm, register_d_model
    NR.offline(monkeypatch)
    path = str(tmp_path / "llm")
    NR.build_local_llm(path, N_LAYER, D, H, N_POS)
    register_d_model(path, D)
    tok, model = load_llm(path, None, _dev())
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
    before = dict(L.path_calls)
    out, mask = L.embed_notes(WINDOWS, tok, model, max_length=N_POS)
    assert L.path_calls["fused"] == before["fused"] + 1 and L.path_calls["stock"] == before["stock"]
    want, want_mask = _stock(WINDOWS, tok, model)
    assert out.shape == (3, 4, D) and out.is_cuda and mask.is_cuda and torch.equal(mask, want_mask)
    assert mask.tolist() == [[True] * 4, [False] * 4, [True, False, False, False]]
    err = _rel(out, want)
    print(f"embed_notes fused vs stock on the GPU: {err:.2e}")
    assert err < BAR
    assert not out[0, 1].any() and not out[1].any() and not out[2, 1:].any()


def test_a_left_padding_tokenizer_takes_the_stock_path(llm, tmp_path):
    from fusions import load_llm as L
    _, _, model = llm
    tok = NR.build_tokenizer(str(tmp_path / "left"), padding_side="left")
    tok.pad_token = tok.eos_token
    before = dict(L.path_calls)
    with torch.no_grad():
        out, _ = L.embed_notes([["seen at noon", "x" * 40]], tok, model, max_length=N_POS)
    assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("which", ["TTF_T2V_XAttn", "TTF_RecAvg"])
def test_raw_text_mode_equals_the_precomputed_path(llm, which):
    import importlib

    from fusions.load_llm import embed_notes
    from immtsf.ops import PackedNotes
    path, tok, model = llm
    dev = _dev()
    cls = getattr(importlib.import_module(f"fusions.{which}"), which)
    extra = dict(n_heads_fusion=2) if which == "TTF_T2V_XAttn" else dict(recency_sigma=1.0)
    torch.manual_seed(3)
    raw = cls(path, None, max_length=N_POS, device=str(dev), use_text_embeddings=False, dropout=0.1, d_txt=64, **extra).to(dev).eval()
    pre = cls(path, None, max_length=N_POS, device=str(dev), use_text_embeddings=True, dropout=0.1, d_txt=64, **extra).to(dev).eval()
    pre.load_state_dict({k: v for k, v in raw.state_dict().items() if not k.startswith("llm_model.")})
    g = torch.Generator().manual_seed(4)
    tau = (torch.rand(3, 4, generator=g) * 24).to(dev)
    t_hat = torch.sort(torch.rand(3, 5, generator=g), 1).values.to(dev)
    E, M = raw(WINDOWS, tau, t_hat)
    V, mask = embed_notes(WINDOWS, tok, model, max_length=N_POS)
    if which == "TTF_T2V_XAttn":       # the note mask is the lists': the precomputed path takes it as PackedNotes' lengths
        rows = V[mask]
        fed = PackedNotes(rows, torch.arange(rows.shape[0], dtype=torch.int32, device=dev), mask.sum(1).to(torch.int32), 4)
    else:
        fed = V
    E_want, _ = pre(fed, tau, t_hat)
    err = _rel(E, E_want)
    print(f"{which}: raw-text vs precomputed E_txt {err:.2e}")
    assert E.shape == (3, 5, 64) and err < BAR
    assert M.dtype == torch.bool and M.view(-1).tolist() == [True, False, True]
    trainable = [k for k, p in raw.named_parameters() if p.requires_grad]
    assert trainable and not any(k.startswith("llm_model.") for k in trainable)
    assert all(not p.requires_grad for p in raw.llm_model.parameters())
    listed = raw._params() if which == "TTF_RecAvg" else [p for grp in raw.grad_phases() for p in grp]
    frozen = {id(p) for p in raw.llm_model.parameters()}
    assert not any(id(p) in frozen for p in listed if p is not None)
    assert not raw.train().llm_model.training


def test_embed_corpus_keeps_input_order_over_three_launches(llm):
    from fusions import load_llm as L
    from immtsf import config
    from immtsf.text import embed_corpus, plan_batches
    _, tok, model = llm
    notes = ["x" * 60, "seen at noon", "", "y" * 70, "blood pressure stable", "z" * 50, "a"]
    counts = [60, 12, 0, 70, 21, 50, 1]
    assert len(plan_batches(counts, 96)) == 3
    before = dict(L.path_calls)
    out = embed_corpus(notes, tok, model, max_length=N_POS, tokens_per_batch=96)
    # (five notes, one, one: in fp32 mode a single-note launch takes the padded call, config.note_embed_fp32_min_notes)
    assert L.path_calls["fused"] == before["fused"] + 1 and L.path_calls["stock"] == before["stock"] + 2
    config.precision = "bf16"
    before = dict(L.path_calls)
    out16 = embed_corpus(notes, tok, model, max_length=N_POS, tokens_per_batch=96)
    config.precision = "fp32"
    assert L.path_calls["fused"] == before["fused"] + 3 and L.path_calls["stock"] == before["stock"]
    assert float((out16 - out).abs().max()) / float(out.abs().max()) < 4.0 * _autocast_error("edges") + BAR
    assert out.shape == (7, D) and not out.is_cuda
    scale = float(out.abs().max())
    for i, note in enumerate(notes):
        one, _ = L.embed_notes([[note]], tok, model, max_length=N_POS)
        assert float((one[0, 0].cpu() - out[i]).abs().max()) / scale < BAR, i
