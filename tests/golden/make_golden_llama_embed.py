#!/usr/bin/env python3
"""Generate tests/golden/llama_embed.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE): fusions/load_llm.py embed_notes on
the CPU, fp32, over a tiny local LlamaModel (2 layers, 64 wide, 2 heads over 1 K/V head -- head_dim 32 --, intermediate 128, llama3 RoPE
with original_max_position_embeddings 8, max_position_embeddings = max_length = 24) behind the tokenizer of tests/llama_embed_ref.py.

    IMMTSF_REFERENCE=/path/to/reference python tests/golden/make_golden_llama_embed.py

Windows: three notes (one of them the empty string), no note at all, one note longer than max_length (truncated) -- so N_max pads two
windows with empty strings, which this tokenizer gives one token (begin of text): their rows are not zero in the reference.  The
tokenizer has no pad token; it gets the end-of-text token, as the reference's load_llm gives it.  The reference module is imported
unmodified at run time; the file stores tensors and the notes' text only: the token ids and attention mask the tokenizer returned, the
model's weights (`w.`) and its rotary inv_freq / attention_scaling, the reference's output and note mask: data, no code."""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import llama_embed_ref as LR  # noqa: E402

N_LAYER, D, H, H_KV, INNER, N_POS = 2, 64, 2, 1, 128, 24
NOTES = [["seen at noon", "", "blood pressure stable"], [], ["river level rising after heavy rain, plan unchanged " * 3]]


def main():
    ref_root = os.environ["IMMTSF_REFERENCE"]
    spec = importlib.util.spec_from_file_location("reference_load_llm", os.path.join(ref_root, "fusions", "load_llm.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory() as tmp:
        tok, model = LR.build_local_llama(tmp, N_LAYER, D, H, H_KV, INNER, N_POS)
    tok.pad_token = tok.eos_token
    torch.manual_seed(0)
    with torch.no_grad():
        out, note_mask = ref.embed_notes(NOTES, tok, model, max_length=N_POS)
    n_max = max(len(w) for w in NOTES)
    enc = tok([n for w in NOTES for n in w + [""] * (n_max - len(w))], padding="max_length", truncation=True, max_length=N_POS,
              return_tensors="pt")
    fixture = {"input_ids": enc.input_ids.numpy(), "attention_mask": enc.attention_mask.numpy(), "out": out.numpy(),
               "note_mask": note_mask.numpy(), "notes_json": np.array(json.dumps(NOTES)),
               "dims": np.array([N_LAYER, D, H, H_KV, INNER, N_POS, len(tok)], dtype=np.int64)}
    for k, v in LR.weights64(model).items():
        fixture["w." + k] = v.float().numpy()
    path = os.path.join(HERE, "llama_embed.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes; token counts", enc.attention_mask.sum(1).tolist())


if __name__ == "__main__":
    main()
