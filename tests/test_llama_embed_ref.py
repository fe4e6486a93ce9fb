"""CPU checks of raw-text mode's Llama path.
  * the exactness claim the kernels rely on: the float64 restatement over the RAGGED tokens (tests/llama_embed_ref.py) equals the padded
    call LlamaModel.double()(input_ids, attention_mask) + masked mean-pool at 1e-10 relative to the largest element (the bar of
    tests/test_note_embed_ref.py), with notes of 0 (ids given directly), 1, 2 and 12 tokens and a truncated one, for rope_type default
    and llama3 (original_max_position_embeddings 8, below the longest note: the rescaled bands are in play) and for G = 1 and G = 2.
    transformers takes the rotary angles AND every RMSNorm in fp32 even in a .double() model; the restatement follows both for this pin
  * the golden written by tests/golden/make_golden_llama_embed.py from the reference's real embed_notes (fp32, CPU): the restatement and
    fusions.load_llm.embed_notes (stock path on the CPU) match its output at 1e-5 and its note mask exactly
  * load_llm on a local Llama directory gives the tokenizer the end-of-text token as its pad token and keeps every layer
The tokenizer and models are built in a temporary directory by the tests; nothing is fetched."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llama_embed_ref as LR  # noqa: E402


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.fixture()
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "llama_embed.npz"))


@pytest.mark.parametrize("rope", ["default", "llama3"])
@pytest.mark.parametrize("n_kv", [2, 1])                 # G = 1, G = 2
def test_ragged_restatement_equals_the_padded_call(monkeypatch, rope, n_kv):
    LR.offline(monkeypatch)
    tok = LR.build_tokenizer(None)
    tok.pad_token = tok.eos_token
    model = LR.build_llama(None, len(tok), n_layer=2, hidden=64, n_head=2, n_kv=n_kv, inner=128, max_pos=24,
                           rope=LR.DEFAULT_ROPE if rope == "default" else LR.LLAMA3_ROPE)
    assert model.rotary_emb.rope_type == rope
    notes = ["", "a", "abcdefghijk", "river level rising after heavy rain, plan unchanged " * 3]      # 1, 2, 12, > 24 -> 24 tokens
    enc = tok(notes, padding="max_length", truncation=True, max_length=24, return_tensors="pt")
    assert enc.attention_mask.sum(1).tolist() == [1, 2, 12, 24] and tok.padding_side == "right"
    # a note of no tokens: no string gives one behind the begin-of-text token, so its row is given directly (all pad)
    ids = torch.cat([enc.input_ids, torch.full((1, 24), tok.pad_token_id, dtype=torch.long)])
    attn = torch.cat([enc.attention_mask, torch.zeros(1, 24, dtype=torch.long)])
    assert attn.sum(1).tolist() == [1, 2, 12, 24, 0]
    w = LR.weights64(model)
    if rope == "llama3":             # the rescaled bands: the low frequencies are divided by the factor, the highest is left alone
        base = 1.0 / (500000.0 ** (torch.arange(0, 32, 2, dtype=torch.float32) / 32))
        assert torch.allclose(w["rotary_emb.inv_freq"][-1], base[-1] / 8.0) and not torch.allclose(w["rotary_emb.inv_freq"], base / 8.0)
    with torch.no_grad():
        padded = LR.pool_padded(model.double(), ids, attn)
    # LlamaModel.double() is not float64 throughout: LlamaRotaryEmbedding forms its angles in fp32 and LlamaRMSNorm casts each row to
    # fp32 (1e-7 apart from a float64 norm).  The restatement follows both here (norm32), so that what the pin measures is the claim
    # itself -- the ragged tokens give the padded call's result -- at the float64 bar; with its float64 norm, the form the kernels are
    # measured against, it stays within fp32 rounding of the same output.
    eps = model.config.rms_norm_eps
    ragged = LR.embed_ragged(w, LR.ragged_from_padded(ids, attn), 2, 2, n_kv, eps, norm32=True)
    err = _rel(ragged, padded)
    err64 = _rel(LR.embed_ragged(w, LR.ragged_from_padded(ids, attn), 2, 2, n_kv, eps), padded)
    print(f"{rope}, G = {2 // n_kv}: ragged restatement vs padded float64 call: {err:.2e}; with float64 norms {err64:.2e}")
    assert err < 1e-10
    assert err64 < 1e-5              # (fp32 rounding of 64-wide rows through 5 norms: the bar of the fp32 golden below)
    assert torch.equal(ragged[4], torch.zeros(64, dtype=torch.float64)) and torch.isfinite(padded).all()
    assert torch.equal(padded[4], torch.zeros(64, dtype=torch.float64))            # an all-masked row stays finite and pools to 0


def _golden_weights(golden, dtype):
    w = {k[2:]: torch.from_numpy(golden[k]).to(dtype) for k in golden.files if k.startswith("w.") and "rotary_emb" not in k}
    rot = {k[2:]: torch.from_numpy(golden[k]) for k in golden.files if k.startswith("w.rotary_emb")}
    return w, rot


def test_ragged_restatement_matches_the_reference_golden(golden):
    n_layer, d, H, H_kv, inner, n_pos, vocab = (int(v) for v in golden["dims"])
    w, rot = _golden_weights(golden, torch.float64)
    ids, attn = torch.from_numpy(golden["input_ids"]), torch.from_numpy(golden["attention_mask"])
    counts = attn.sum(1).tolist()
    assert n_pos in counts and counts.count(1) >= 3                 # a truncated note; the padded-out notes are the begin-of-text token
    ragged = LR.embed_ragged({**w, **rot}, LR.ragged_from_padded(ids, attn), n_layer, H, H_kv)
    want = torch.from_numpy(golden["out"])
    err = _rel(ragged.view(want.shape), want)
    print(f"ragged restatement vs the reference's fp32 output: {err:.2e}")
    assert err < 1e-5


def test_embed_notes_on_the_cpu_matches_the_reference_golden(golden, monkeypatch):
    from transformers import LlamaModel

    from fusions import load_llm as L
    LR.offline(monkeypatch)
    n_layer, d, H, H_kv, inner, n_pos, vocab = (int(v) for v in golden["dims"])
    tok = LR.build_tokenizer(None)
    tok.pad_token = tok.eos_token
    assert len(tok) == vocab
    model = LlamaModel(LR.llama_config(vocab, n_layer, d, H, H_kv, inner, n_pos)).eval()
    w, rot = _golden_weights(golden, torch.float32)
    model.load_state_dict(w)
    assert torch.equal(model.rotary_emb.inv_freq, rot["rotary_emb.inv_freq"])      # the config rebuilds the fixture's frequencies
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


def test_load_llm_on_a_local_llama(tmp_path, monkeypatch):
    from fusions.load_llm import load_llm
    LR.offline(monkeypatch)
    path = str(tmp_path / "llama")
    LR.build_local_llama(path, n_layer=3, hidden=64, n_head=2, n_kv=1, inner=128, max_pos=24)
    tok, model = load_llm(path, 2, "cpu")
    assert type(model).__name__ == "LlamaModel" and len(model.layers) == 3          # (only an encoder.layer stack is cut, as in the reference)
    assert tok.pad_token == LR.EOS and tok.pad_token_id == 1 and tok.padding_side == "right"
    assert tok("").input_ids == [0] and len(tok("abc").input_ids) == 4
    assert model.get_input_embeddings().weight.shape[0] == len(tok)
    assert all(not p.requires_grad for p in model.parameters())
    assert next(model.parameters()).device.type == "cpu"
