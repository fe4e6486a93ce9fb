"""float64 restatement of raw-text mode's note embedding over the RAGGED tokens -- each note's real tokens through the GPT-2 body on its
own (tests/gpt2_ref.py: no padding, no attention mask), then the mean over its rows; a note of no tokens is a zero row -- and the
builders of the local tokenizer / model directories the raw-text tests load (no test names a hub model).
tests/test_note_embed_ref.py pins the restatement to the padded call of the installed GPT2Model; the GPU tests compare the kernels
with it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpt2_ref as R  # noqa: E402

weights64 = R.weights64

CORPUS = ["the patient was seen at noon", "blood pressure stable overnight", "no acute distress, plan unchanged",
          "river level rising after heavy rain", "0123456789 .,;:-"]


def embed_ragged(w, notes_ids, n_layer, n_head, eps=1e-5):
    """notes_ids: a list of N lists of token ids -> (N, d) float64"""
    d = w["wte.weight"].shape[1]
    out = torch.zeros(len(notes_ids), d, dtype=torch.float64)
    for n, ids in enumerate(notes_ids):
        if len(ids):
            x = w["wte.weight"][torch.as_tensor(ids, dtype=torch.long)].unsqueeze(0)
            out[n] = R.body(w, x, n_layer, n_head, eps)[0].mean(dim=0)
    return out


def ragged_from_padded(input_ids, attention_mask):
    """the real tokens of each row of a right-padded batch"""
    return [row[:int(m.sum())].tolist() for row, m in zip(input_ids, attention_mask)]


def pool_padded(model, input_ids, attention_mask):
    """the reference's formulation on `model` as it stands (dtype and device of its parameters)"""
    hidden = model(input_ids=input_ids, attention_mask=attention_mask).last_hidden_state
    keep = attention_mask.unsqueeze(-1)
    return (hidden * keep).sum(dim=1) / keep.sum(dim=1).clamp(min=1)


def offline(monkeypatch):
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    monkeypatch.setenv("TRANSFORMERS_OFFLINE", "1")


def build_tokenizer(path, padding_side="right"):
    """a byte-level BPE trained in place with NO merges (256 byte symbols + the end-of-text token: one token per ASCII character, so a
    test controls every note's token count), wrapped as a fast tokenizer without a pad token and saved to `path`"""
    from tokenizers import ByteLevelBPETokenizer
    from transformers import PreTrainedTokenizerFast
    bpe = ByteLevelBPETokenizer()
    bpe.train_from_iterator(iter(CORPUS), vocab_size=257, min_frequency=1, special_tokens=["<|endoftext|>"], show_progress=False)
    fast = PreTrainedTokenizerFast(tokenizer_object=bpe._tokenizer, eos_token="<|endoftext|>", padding_side=padding_side)
    fast.save_pretrained(path)
    return fast


def build_model(path, vocab, n_layer, n_embd, n_head, n_positions, seed=5):
    """a tiny random GPT2Model (every parameter moved off its init so that no bias or gain is trivial), saved beside the tokenizer"""
    from transformers import GPT2Config, GPT2Model
    torch.manual_seed(seed)
    m = GPT2Model(GPT2Config(vocab_size=vocab, n_embd=n_embd, n_head=n_head, n_layer=n_layer, n_positions=n_positions, bos_token_id=0,
                             eos_token_id=0))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    m.eval()
    if path is not None:
        m.save_pretrained(path)
    return m


def build_local_llm(path, n_layer, n_embd, n_head, n_positions, padding_side="right"):
    tok = build_tokenizer(path, padding_side)
    return tok, build_model(path, len(tok), n_layer, n_embd, n_head, n_positions)
