#!/usr/bin/env python3
"""Raw-text mode's note embedding, fused (fusions.load_llm.embed_notes -> immtsf.ops.gpt2_embed_notes: the real tokens only, packed;
csrc/note_embed.hip + the GEMM family) against IMMTSF_NOTE_EMBED_FUSED=0 (the reference's formulation: every note padded to max_length,
transformers' GPT2Model on stock PyTorch, masked mean), on the same GPU.  Shape: GPT-2 small (12 layers, 768 wide, 12 heads, random
weights, max_length 1024) behind a stand-in tokenizer (one token per byte, right-padded).  Two workloads, the note lengths printed:
  batch : one embed_notes call over `--notes` notes of mixed length (most short, a few long, one of 1024 tokens)
  single: the same notes one call each, as the reference's compute_text_embeddings.py makes them
The stock path runs the batch in slices of `--stock-slice` notes (a padded batch of all of them does not fit a sensible budget); the
row-count ratio sum(L) / (N * max_length) -- what the algorithm alone saves -- is printed beside the times.  In ONE process, after
warming both paths: `--passes` alternating passes, host clock around a pass with a synchronise at its end.  One JSON line per
precision mode: milliseconds per workload, best pass and all passes (their spread is the noise).
--model bert: the same two workloads on a BERT-base body (768 wide, 12 heads, intermediate 3072, random weights) cut to 6 layers as
load_llm cuts it at the default llm_layers_fusion, max_length 512, behind a WordPiece stand-in ([CLS], one token per character, [SEP],
right-padded) -> immtsf.ops.bert_embed_notes; token counts from a few to 512.
--model llama: the widths of Llama-3.1-8B (4096 wide, 32 heads over 8 K/V heads, head_dim 128, intermediate 14336, llama3 RoPE, random
weights) cut to `--layers` layers (default 2: the whole body is 32 of them and every layer costs the same, so the times scale and the
ratios stand), max_length 1024, the GPT-2 note mix behind a begin-of-text token -> immtsf.ops.llama_embed_notes.

--products split: config.frozen_products = "split" for the whole run -- in fp32 mode the fused operator forms its weight products on
the split-bf16 kernel (csrc/gemm_split.hip); bf16 mode and the stock side do not read it.  The same lines, with "products".

--stored bf16 (with --model llama): every parameter of the body cast to bf16 as from_pretrained leaves a bf16 checkpoint (buffers
untouched) and config.llama_stored_bf16 on -- the fused operator reads the checkpoint in place and the stock side is
transformers' padded call OF THE SAME bf16 MODEL, in both precision modes.  Every line also carries each side's peak allocated memory
(torch.cuda.max_memory_allocated over its timed passes, MiB, the model included).

usage: python tools/note_embed_bench.py [--model gpt2|bert|llama] [--products fp32|split] [--stored fp32|bf16] [--layers 2] [--notes 32]
                                        [--passes 3] [--single 8] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MAX_LENGTH = 1024


class ByteTokenizer:
    """stand-in: one token per byte (ids < 256), right-padded to max_length with the pad id, with the attention mask; frame = (first id,
    last id): the WordPiece stand-in, every note between [CLS] and [SEP] (truncation keeps the [SEP]); last id None: the Llama stand-in,
    the begin-of-text token in front only"""
    padding_side = "right"

    def __init__(self, frame=None):
        self.frame = frame

    def __call__(self, texts, padding="max_length", truncation=True, max_length=MAX_LENGTH, return_tensors="pt"):
        import torch
        ids = torch.zeros(len(texts), max_length, dtype=torch.long)
        attn = torch.zeros(len(texts), max_length, dtype=torch.long)
        for r, t in enumerate(texts):
            b = list(t.encode("utf-8"))[:max_length]
            if self.frame:
                tail = [] if self.frame[1] is None else [self.frame[1]]
                b = [self.frame[0]] + b[:max_length - 1 - len(tail)] + tail
            ids[r, :len(b)] = torch.tensor(b, dtype=torch.long)
            attn[r, :len(b)] = 1
        return type("Enc", (), {"input_ids": ids, "attention_mask": attn})()


def note_lengths(n, cap=MAX_LENGTH):
    """most notes short (tens of tokens), some a few hundred, one at the cap"""
    base = [24, 48, 40, 96, 64, 200, 32, 56, 80, 320, 28, 72, 44, 150, 36 if cap == MAX_LENGTH else 6, cap]
    return [base[i % len(base)] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("gpt2", "bert", "llama"), default="gpt2")
    ap.add_argument("--products", choices=("fp32", "split"), default="fp32", help="config.frozen_products for the run (read in fp32 mode)")
    ap.add_argument("--stored", choices=("fp32", "bf16"), default="fp32", help="dtype the --model llama body is stored in")
    ap.add_argument("--layers", type=int, default=2, help="layers of the --model llama body")
    ap.add_argument("--notes", type=int, default=32)
    ap.add_argument("--single", type=int, default=8, help="notes of the one-call-per-note workload (the first ones of the mix)")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--stock-slice", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stored == "bf16" and args.model != "llama":
        ap.error("--stored bf16 needs --model llama")
    import torch
    from transformers import BertConfig, BertModel, GPT2Config, GPT2Model, LlamaConfig, LlamaModel

    from fusions import load_llm as L
    from immtsf import config
    dev = torch.device("cuda:0")
    config.frozen_products = args.products
    torch.manual_seed(0)
    if args.model == "bert":
        max_length, layers = 512, 6
        model = BertModel(BertConfig(vocab_size=258, num_hidden_layers=layers, pad_token_id=0), add_pooling_layer=False)
        tok = ByteTokenizer(frame=(256, 257))
        lengths = note_lengths(args.notes, max_length)
        notes = [chr(97 + i % 26) * (n - 2) for i, n in enumerate(lengths)]
    elif args.model == "llama":
        max_length, layers = MAX_LENGTH, args.layers
        cfg = LlamaConfig(vocab_size=257, hidden_size=4096, num_hidden_layers=layers, num_attention_heads=32, num_key_value_heads=8,
                          intermediate_size=14336, max_position_embeddings=131072, bos_token_id=256, eos_token_id=0, pad_token_id=None,
                          rope_parameters={"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "low_freq_factor": 1.0,
                                           "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
        with torch.device(dev):            # (a layer is 218 M parameters: initialised on the device)
            model = LlamaModel(cfg)
        tok = ByteTokenizer(frame=(256, None))
        lengths = note_lengths(args.notes)
        notes = [chr(97 + i % 26) * (n - 1) for i, n in enumerate(lengths)]
    else:
        max_length, layers = MAX_LENGTH, 12
        model = GPT2Model(GPT2Config(vocab_size=256, bos_token_id=0, eos_token_id=0))
        tok = ByteTokenizer()
        lengths = note_lengths(args.notes)
        notes = [chr(97 + i % 26) * n for i, n in enumerate(lengths)]
    model = model.requires_grad_(False).to(dev).eval()
    if args.stored == "bf16":
        for p in model.parameters():
            p.data = p.data.to(torch.bfloat16)
        config.llama_stored_bf16 = True
    ratio = sum(lengths) / (len(lengths) * max_length)
    print(f"note lengths (tokens): {lengths}", flush=True)
    print(f"rows: real {sum(lengths)} of padded {len(lengths) * max_length} (ratio {ratio:.4f})", flush=True)

    def batch(fused):
        config.note_embed_fused = fused
        with torch.no_grad():
            if fused:
                L.embed_notes([notes], tok, model, max_length=max_length)
            else:
                for i in range(0, len(notes), args.stock_slice):
                    L.embed_notes([notes[i:i + args.stock_slice]], tok, model, max_length=max_length)

    def single(fused):
        config.note_embed_fused = fused
        with torch.no_grad():
            for note in notes[:args.single]:
                L.embed_notes([[note]], tok, model, max_length=max_length)

    def timed(fn):
        """(milliseconds, peak allocated MiB) of one pass"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20

    lines = []
    for prec in ("fp32", "bf16"):
        config.precision = prec
        line = {"tool": "note_embed_bench", "model": args.model, "precision": prec, "products": args.products, "stored": args.stored,
                "layers": layers, "d": int(getattr(model.config, "hidden_size", 768)), "max_length": max_length,
                "notes": len(notes), "row_ratio": round(ratio, 4), "single_notes": args.single, "single_row_ratio":
                round(sum(lengths[:args.single]) / (args.single * max_length), 4), "passes": args.passes}
        for what, fn in (("batch", batch), ("single", single)):
            for fused in (True, False):
                fn(fused)
            t, peak = {True: [], False: []}, {True: 0.0, False: 0.0}
            for _ in range(args.passes):
                for fused in (True, False):
                    ms, mib = timed(lambda: fn(fused))
                    t[fused].append(ms)
                    peak[fused] = max(peak[fused], mib)
            for fused, name in ((True, "fused"), (False, "stock")):
                line[f"{what}_{name}_ms"] = round(min(t[fused]), 3)
                line[f"{what}_{name}_ms_passes"] = [round(v, 3) for v in t[fused]]
                line[f"{what}_{name}_peak_mib"] = round(peak[fused], 1)
            line[f"{what}_speedup"] = round(min(t[False]) / min(t[True]), 2)
        config.note_embed_fused = True
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
