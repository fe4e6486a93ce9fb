#!/usr/bin/env python3
"""One SHA-256 per case over what the frozen-LLM drivers of immtsf.ops return: the three TimeLLM bodies (gpt2_body, bert_body, llama_body:
the output bytes, then the tail-gradient bytes) and the three note embedders (gpt2 / bert / llama_embed_notes: the pooled bytes).  The
kernels have no atomics and a rerun repeats bit for bit, so two checkouts that print the same lines drive the kernels the same way: a
host-side refactor of the drivers is held to byte equality with this.  Only the public front ends are called, so the same file runs on
an older checkout (copy it there, or give --repo).

Bodies: the smallest the predicates accept, offline and randomly initialised from a fixed torch seed (GPT-2 and BERT 64 wide with one
head; Llama with head_dim 128 and H / H_kv of 1 and 2), B = 2, S_t = 3, S_p in {0, 5}, 1 and 3 layers (first is last; first / middle /
last).  Modes: fp32, fp32 with config.frozen_products = "split", bf16.  GPT-2 and BERT run in training mode with dropout 0.1 and an
explicit seed.  Notes (on the 3-layer bodies): five notes of 3, 0, 1, 7 and 2 tokens; five empty notes; no note at all.

usage: python tools/llm_driver_digest.py [--repo DIR] [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import torch

SEED, DROP_SEED, P_DROP = 20, 1234, 0.1
B, S_T, PREFIXES, LAYERS = 2, 3, (0, 5), (1, 3)
MODES = (("fp32", "fp32", "fp32"), ("split", "fp32", "split"), ("bf16", "bf16", "fp32"))      # name, precision, frozen_products
NOTES = (("mixed", (3, 0, 1, 7, 2)), ("all_empty", (0, 0, 0, 0, 0)), ("no_note", ()))
N_POS, VOCAB = 16, 32


def _models():
    """name -> (build(n_layer), body front end's name, trained with dropout)"""
    from transformers import BertConfig, BertModel, GPT2Config, GPT2Model, LlamaConfig, LlamaModel

    def moved(m):        # every parameter off its init, so that no bias or gain is trivial
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        return m.requires_grad_(False)

    def gpt2(n):
        return moved(GPT2Model(GPT2Config(n_embd=64, n_head=1, n_layer=n, n_positions=N_POS, vocab_size=VOCAB, bos_token_id=0,
                                          eos_token_id=0, resid_pdrop=P_DROP, embd_pdrop=P_DROP, attn_pdrop=P_DROP))).train()

    def bert(n):
        return moved(BertModel(BertConfig(vocab_size=VOCAB, hidden_size=64, num_hidden_layers=n, num_attention_heads=1, intermediate_size=128,
                                          max_position_embeddings=N_POS, pad_token_id=0, hidden_dropout_prob=P_DROP,
                                          attention_probs_dropout_prob=P_DROP), add_pooling_layer=False)).train()

    def llama(H, H_kv):
        def build(n):
            return moved(LlamaModel(LlamaConfig(vocab_size=VOCAB, hidden_size=128 * H, num_hidden_layers=n, num_attention_heads=H,
                                                num_key_value_heads=H_kv, intermediate_size=256, max_position_embeddings=N_POS, head_dim=128,
                                                rope_parameters={"rope_type": "default", "rope_theta": 10000.0}, bos_token_id=0,
                                                eos_token_id=1, pad_token_id=None))).eval()
        return build

    return {"gpt2": (gpt2, "gpt2", True), "bert": (bert, "bert", True), "llama_g1": (llama(1, 1), "llama", False),
            "llama_g2": (llama(2, 1), "llama", False)}


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose immtsf runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for p in (args.repo, os.path.join(args.repo, "imm-tsf_amd")):
        sys.path.insert(0, p)
    from immtsf import config, ops
    dev = torch.device("cuda:0")
    lines = []

    def emit(name, digest):
        lines.append(f"{name} {digest}")
        print(lines[-1], flush=True)

    for name, (build, kind, train) in _models().items():
        for n_layer in LAYERS:
            torch.manual_seed(SEED)
            model = build(n_layer).to(dev)
            d = model.config.hidden_size
            body = getattr(ops, kind + "_body")
            for S_p in PREFIXES:
                g = torch.Generator().manual_seed(100 + S_p)
                prefix, tail0, up = (torch.randn(B, n, d, generator=g).to(dev) for n in (S_p, S_T, S_T))
                for mode, precision, products in MODES:
                    config.frozen_products = products
                    tail = tail0.clone().requires_grad_(True)
                    kw = dict(precision=precision, seed=DROP_SEED) if train else dict(precision=precision)
                    out = body(model, prefix, tail, train, **kw)
                    (out * up).sum().backward()
                    emit(f"body {name} L{n_layer} Sp{S_p} {mode}", _sha(out, tail.grad))
            if n_layer != LAYERS[-1]:
                continue
            embed = getattr(ops, kind + "_embed_notes")
            for what, lengths in NOTES:
                g = torch.Generator().manual_seed(7)
                ids = torch.randint(0, VOCAB, (sum(lengths),), generator=g).to(torch.int32).to(dev)
                cu = torch.tensor([sum(lengths[:i]) for i in range(len(lengths) + 1)], dtype=torch.int32, device=dev)
                for mode, precision, products in MODES:
                    config.frozen_products = products
                    pooled = embed(model.eval(), ids, cu, precision=precision)
                    assert tuple(pooled.shape) == (len(lengths), d)
                    emit(f"notes {name} {what} {mode}", _sha(pooled))
    config.frozen_products = "fp32"
    torch.cuda.synchronize()
    emit("all", hashlib.sha256("\n".join(lines).encode()).hexdigest())
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
