"""CPU checks of raw-text mode.
  * the exactness claim the kernels rely on: the float64 restatement over the RAGGED tokens (tests/note_embed_ref.py) equals the padded
    call GPT2Model.double()(input_ids, attention_mask) + masked mean-pool at 1e-10 relative to the largest element (the bar of
    tests/test_gpt2_ref.py), with a note of no tokens and a note truncated at max_length
  * the golden written by tests/golden/make_golden_note_embed.py from the reference's real embed_notes (fp32, CPU): the restatement and
    fusions.load_llm.embed_notes (stock path on the CPU) match its output at 1e-5 and its note mask exactly
  * load_llm on a local directory; the corpus helper's batch plan
The tokenizer and models are built in a temporary directory by the tests; nothing is fetched."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import note_embed_ref as NR  # noqa: E402


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture()
def local_llm(tmp_path, monkeypatch):
    NR.offline(monkeypatch)
    path = str(tmp_path / "llm")
    NR.build_local_llm(path, n_layer=2, n_embd=64, n_head=1, n_positions=24)
    return path


@pytest.fixture()
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "note_embed.npz"))


def test_ragged_restatement_equals_the_padded_call(tmp_path, monkeypatch):
    NR.offline(monkeypatch)
    tok = NR.build_tokenizer(str(tmp_path / "tok"))
    tok.pad_token = tok.eos_token
    model = NR.build_model(None, len(tok), n_layer=2, n_embd=64, n_head=1, n_positions=24)
    notes = ["", "a", "seen at noon", "x" * 24, "blood pressure stable overnight, plan unchanged"]       # 0, 1, 12, 24, 47 -> 24 tokens
    enc = tok(notes, padding="max_length", truncation=True, max_length=24, return_tensors="pt")
    assert enc.attention_mask.sum(1).tolist() == [0, 1, 12, 24, 24]
    with torch.no_grad():
        padded = NR.pool_padded(model.double(), enc.input_ids, enc.attention_mask)
    ragged = NR.embed_ragged(NR.weights64(model), NR.ragged_from_padded(enc.input_ids, enc.attention_mask), 2, 1,
                             model.config.layer_norm_epsilon)
    err = _rel(ragged, padded)
    print(f"ragged restatement vs padded float64 call: {err:.2e}")
    assert err < 1e-10
    assert torch.equal(ragged[0], torch.zeros(64, dtype=torch.float64)) and torch.isfinite(padded).all()


def test_ragged_restatement_matches_the_reference_golden(golden):
    n_layer, d, H, n_pos, vocab = (int(v) for v in golden["dims"])
    w = {k[2:]: torch.from_numpy(golden[k]).double() for k in golden.files if k.startswith("w.")}
    ids, attn = torch.from_numpy(golden["input_ids"]), torch.from_numpy(golden["attention_mask"])
    assert 0 in attn.sum(1).tolist() and n_pos in attn.sum(1).tolist()          # a note of no tokens and a truncated one
    ragged = NR.embed_ragged(w, NR.ragged_from_padded(ids, attn), n_layer, H)
    want = torch.from_numpy(golden["out"])
    err = _rel(ragged.view(want.shape), want)
    print(f"ragged restatement vs the reference's fp32 output: {err:.2e}")
    assert err < 1e-5


def test_embed_notes_on_the_cpu_matches_the_reference_golden(golden, tmp_path, monkeypatch):
    from transformers import GPT2Config, GPT2Model

    from fusions import load_llm as L
    NR.offline(monkeypatch)
    n_layer, d, H, n_pos, vocab = (int(v) for v in golden["dims"])
    tok = NR.build_tokenizer(str(tmp_path / "tok"))
    tok.pad_token = tok.eos_token
    assert len(tok) == vocab
    model = GPT2Model(GPT2Config(vocab_size=vocab, n_embd=d, n_head=H, n_layer=n_layer, n_positions=n_pos)).eval()
    model.load_state_dict({k[2:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("w.")})
    notes = json.loads(str(golden["notes_json"]))
    assert any(len(w) == 0 for w in notes) and len({len(w) for w in notes}) > 1          # an empty window, N_max padding
    before = dict(L.path_calls)
    with torch.no_grad():
        out, mask = L.embed_notes(notes, tok, model, max_length=n_pos)
    assert L.path_calls["stock"] == before["stock"] + 1 and L.path_calls["fused"] == before["fused"]
    want = torch.from_numpy(golden["out"])
    assert out.shape == want.shape and mask.dtype == torch.bool
    assert torch.equal(mask, torch.from_numpy(golden["note_mask"]))
    err = _rel(out, want)
    print(f"embed_notes (stock path, CPU) vs the reference: {err:.2e}")
    assert err < 1e-5


def test_load_llm_from_a_local_directory(local_llm):
    from fusions.load_llm import load_llm
    tok, model = load_llm(local_llm, 1, "cpu")
    assert tok.pad_token is not None and tok.pad_token == tok.eos_token
    assert model.get_input_embeddings().weight.shape[0] == len(tok)
    assert len(model.h) == 2                                            # a GPT-2 keeps its blocks: only encoder.layer is cut
    assert all(not p.requires_grad for p in model.parameters())
    assert next(model.parameters()).device.type == "cpu"


def test_embed_notes_without_notes(local_llm):
    from fusions.load_llm import embed_notes, load_llm
    tok, model = load_llm(local_llm, None, "cpu")
    out, mask = embed_notes([[], []], tok, model, max_length=24)
    assert out.shape == (2, 0, 64) and mask.shape == (2, 0)


def test_corpus_batches_cover_every_note_once_within_the_budget():
    from immtsf.text import plan_batches
    counts = [5, 0, 40, 7, 7, 64, 1]
    groups = plan_batches(counts, 16)
    assert sorted(i for g in groups for i in g) == list(range(len(counts)))
    for g in groups:
        assert len(g) == 1 or sum(max(counts[i], 1) for i in g) <= 16
    assert len(groups) >= 3
