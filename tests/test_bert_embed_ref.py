"""CPU checks of raw-text mode's BERT path.
  * the exactness claim the kernels rely on: the float64 restatement over the RAGGED tokens (tests/bert_embed_ref.py) equals the padded
    call BertModel.double()(input_ids, attention_mask) + masked mean-pool at 1e-10 relative to the largest element (the bar of
    tests/test_note_embed_ref.py), with notes of 0 (ids given directly), 1, 2 and mid-length token counts and a truncated one
  * the golden written by tests/golden/make_golden_bert_embed.py from the reference's real embed_notes (fp32, CPU): the restatement and
    fusions.load_llm.embed_notes (stock path on the CPU) match its output at 1e-5 and its note mask exactly
  * load_llm on a local BERT directory cuts the layer stack
The tokenizer and models are built in a temporary directory by the tests; nothing is fetched."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bert_embed_ref as BR  # noqa: E402


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture()
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "bert_embed.npz"))


def test_ragged_restatement_equals_the_padded_call(monkeypatch):
    BR.offline(monkeypatch)
    tok = BR.build_wordpiece_tokenizer(None)
    model = BR.build_bert(None, len(tok), n_layer=2, hidden=64, n_head=1, inner=128, max_pos=24)
    notes = ["", "a b c d e f g h i j", "river level rising after heavy rain , plan unchanged " * 3]      # 2, 12, > 24 -> 24 tokens
    enc = tok(notes, padding="max_length", truncation=True, max_length=24, return_tensors="pt")
    assert enc.attention_mask.sum(1).tolist() == [2, 12, 24] and tok.padding_side == "right"
    # notes of 0 and 1 tokens: no string gives them behind [CLS] ... [SEP], so their ids are given directly
    ids = torch.cat([enc.input_ids, torch.zeros(2, 24, dtype=torch.long)])
    attn = torch.cat([enc.attention_mask, torch.zeros(2, 24, dtype=torch.long)])
    ids[4, 0], attn[4, 0] = 7, 1
    assert attn.sum(1).tolist() == [2, 12, 24, 0, 1]
    with torch.no_grad():
        padded = BR.pool_padded(model.double(), ids, attn)
    ragged = BR.embed_ragged(BR.weights64(model), BR.ragged_from_padded(ids, attn), 2, 1, model.config.layer_norm_eps)
    err = _rel(ragged, padded)
    print(f"ragged restatement vs padded float64 call: {err:.2e}")
    assert err < 1e-10
    assert torch.equal(ragged[3], torch.zeros(64, dtype=torch.float64)) and torch.isfinite(padded).all()
    assert torch.equal(padded[3], torch.zeros(64, dtype=torch.float64))            # an all-masked row stays finite and pools to 0


def test_ragged_restatement_matches_the_reference_golden(golden):
    n_layer, d, H, inner, n_pos, vocab = (int(v) for v in golden["dims"])
    w = {k[2:]: torch.from_numpy(golden[k]).double() for k in golden.files if k.startswith("w.")}
    ids, attn = torch.from_numpy(golden["input_ids"]), torch.from_numpy(golden["attention_mask"])
    counts = attn.sum(1).tolist()
    assert n_pos in counts and counts.count(2) >= 3                 # a truncated note; the padded-out notes are [CLS] [SEP]
    ragged = BR.embed_ragged(w, BR.ragged_from_padded(ids, attn), n_layer, H)
    want = torch.from_numpy(golden["out"])
    err = _rel(ragged.view(want.shape), want)
    print(f"ragged restatement vs the reference's fp32 output: {err:.2e}")
    assert err < 1e-5


def test_embed_notes_on_the_cpu_matches_the_reference_golden(golden, monkeypatch):
    from transformers import BertModel

    from fusions import load_llm as L
    BR.offline(monkeypatch)
    n_layer, d, H, inner, n_pos, vocab = (int(v) for v in golden["dims"])
    tok = BR.build_wordpiece_tokenizer(None)
    assert len(tok) == vocab
    model = BertModel(BR.bert_config(vocab, n_layer, d, H, inner, n_pos)).eval()
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
    assert out[1].abs().max() > 0                                   # the padded-out rows are not zero for this tokenizer
    err = _rel(out, want)
    print(f"embed_notes (stock path, CPU) vs the reference: {err:.2e}")
    assert err < 1e-5


def test_load_llm_cuts_the_layer_stack_of_a_local_bert(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm
    BR.offline(monkeypatch)
    path = str(tmp_path / "bert")
    BR.build_local_bert(path, n_layer=3, hidden=64, n_head=1, inner=128, max_pos=24)
    tok, model = load_llm(path, 2, "cpu")
    assert type(model).__name__ == "BertModel" and len(model.encoder.layer) == 2
    assert tok.pad_token == "[PAD]" and tok.pad_token_id == 0 and tok.padding_side == "right"
    assert model.get_input_embeddings().weight.shape[0] == len(tok)
    assert all(not p.requires_grad for p in model.parameters())
    assert next(model.parameters()).device.type == "cpu"
