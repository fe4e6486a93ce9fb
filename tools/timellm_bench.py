#!/usr/bin/env python3
"""TimeLLM's frozen GPT-2 body, fused (immtsf.ops.gpt2_body: csrc/gpt2.hip + the GEMM family, backward over the patch rows only) against
IMMTSF_TIMELLM_FUSED=0 (transformers' GPT2Model on stock PyTorch, fp32, full autograd), at the shape of `bench.py --config cfg5`: B = 64
windows, a random-init 6-layer GPT-2 (768 wide, 12 heads), input_len = pred_len = 32, C = 8, patches of 16 with stride 8 -- S_t = 32
patch rows behind the prompt the model builds for the batch (its length is printed as S_p).  Two measurements per precision mode (fp32,
bf16): the body alone (forward + backward to the patch rows) and the whole forecasting() + backward.  Eager only: the prompt is built on
the host, so the step cannot be captured.  In ONE process, after warming both paths: `--passes` alternating passes of `--iters` steps
each, host clock around a pass with a synchronise at its end.  Prints one JSON line per mode: milliseconds per step, best pass and all
passes (their spread is the noise).

--llm LLAMA: the same for the frozen Llama body (immtsf.ops.llama_body: csrc/llama_body.hip) on an offline stand-in of huggyllama/llama-7b's
widths (hidden 4096, 32 heads over 32 K/V heads, intermediate 11008) with 2 layers, at the same B, S_p and S_t; the body alone, with
the launches per direction of the fused plan in the line.

--llm BERT: the same for the frozen BERT body (immtsf.ops.bert_body: csrc/bert_body.hip) on an offline stand-in of bert-base's widths
(hidden 768, 12 heads, intermediate 3072; max_position_embeddings 1024 so that the prompt and the patches fit) with 6 layers, at the
same B, S_p and S_t, in train mode (the body's dropouts at BertConfig's 0.1 on both paths); the body alone, with the launches per
direction of the fused plan in the line.

--prompt: the prompt's statistics in one launch and one host copy (immtsf.ops.timellm_prompt_stats: csrc/timellm_prompt.hip) against
IMMTSF_TIMELLM_PROMPT_FUSED=0 (the torch expressions, five host reads per window) with the GPT-2 body fused on both sides, at the same
shape (B 64, L 32, C 8, top_k 5): _get_prompt() alone on the normalised batch and the whole forecasting() + backward, the same
alternating passes; one JSON line per precision mode with the best pass, all passes and their range (lo, hi) per side.

--reprogram: the word prototypes in folded form (immtsf.ops.timellm_prototypes: csrc/timellm_reprogram.hip) against
IMMTSF_TIMELLM_REPROGRAM_FUSED=0 (the mapping layer and the two projections as three linear() calls) with the GPT-2 body fused on both
sides: the stage alone, forward + backward (V 50257, S 1000, d_llm 768, H 8, d_keys 2: the model's own parameters), and the whole
forecasting() + backward, the same alternating passes; one JSON line per precision mode with the best pass, all passes and their range
(lo, hi) per side, whether every pass with the knob on lies below every pass with it off, and the operator's launches per direction.

--products split: config.frozen_products = "split" for the whole run -- in fp32 mode the fused body forms its weight products on the
split-bf16 kernel (csrc/gemm_split.hip); bf16 mode and the stock side do not read it.  The same lines, with "products" in them.

--stored bf16 (with --llm LLAMA): every parameter of the body cast to bf16 as from_pretrained leaves a bf16 checkpoint (buffers
untouched) and config.llama_stored_bf16 on -- the fused body reads the checkpoint in place (fp32 inputs, fp32 result and
gradient) and the stock side is transformers' call OF THE SAME bf16 MODEL on the inputs cast to bf16 (it raises on fp32 inputs_embeds), in
both precision modes.  Every body line also carries each side's peak allocated memory (torch.cuda.max_memory_allocated over its timed
passes, MiB, the model included).

usage: python tools/timellm_bench.py [--llm GPT2|LLAMA|BERT] [--products fp32|split] [--stored fp32|bf16] [--prompt | --reprogram]
                                     [--iters 5] [--passes 5] [--batch 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "imm-tsf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

L, C, LAYERS = 32, 8, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--llm", choices=("GPT2", "LLAMA", "BERT"), default="GPT2")
    ap.add_argument("--products", choices=("fp32", "split"), default="fp32", help="config.frozen_products for the run (read in fp32 mode)")
    ap.add_argument("--stored", choices=("fp32", "bf16"), default="fp32", help="dtype the --llm LLAMA body is stored in")
    ap.add_argument("--prompt", action="store_true", help="time the prompt statistics, knob on against knob off (GPT-2 body)")
    ap.add_argument("--reprogram", action="store_true", help="time the folded word prototypes, knob on against knob off (GPT-2 body)")
    args = ap.parse_args()
    if (args.prompt or args.reprogram) and args.llm != "GPT2":
        ap.error("--prompt / --reprogram run with the GPT-2 body")
    if args.prompt and args.reprogram:
        ap.error("--prompt and --reprogram are separate legs")
    llama, bert = args.llm == "LLAMA", args.llm == "BERT"
    if args.stored == "bf16" and not llama:
        ap.error("--stored bf16 needs --llm LLAMA")
    layers = 2 if llama else LAYERS
    import torch
    from immtsf import config, ops
    from models.TimeLLM import TimeLLM
    dev = torch.device("cuda:0")
    config.frozen_products = args.products
    B = args.batch
    torch.manual_seed(0)
    m = TimeLLM(types.SimpleNamespace(
        input_len=L, pred_len=L, use_norm=True, d_ff=32, ts_vocab_size=1000, input_token_len=16, stride=8, domain_des="synthetic", top_k=5,
        C=C, llm_model_timellm=args.llm, llm_layers_timellm=layers, dropout=0.1, d_model=16, n_heads=8, batch_size=B, device=str(dev),
        immtsf_offline_llm=dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, intermediate_size=11008) if llama
        else dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=1024) if bert
        else True)).to(dev).train()
    if args.stored == "bf16":
        for p in m.llm_model.parameters():
            p.data = p.data.to(torch.bfloat16)
        config.llama_stored_bf16 = True
    m.word_embeddings = m.llm_model.get_input_embeddings().weight
    g = torch.Generator().manual_seed(1)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float().to(dev)
    data = torch.randn(B, L, C, generator=g).to(dev) * mask
    tp = (torch.sort(torch.rand(B, L, generator=g), 1).values * 0.5).to(dev)
    tpp = torch.sort(torch.rand(B, L, generator=g), 1).values.to(dev)
    up = torch.randn(B, L, C, generator=g).to(dev)
    # the body's inputs as forecasting() forms them: the prompt's embeddings (frozen) and S_t reprogrammed patch rows
    from models._common import masked_instance_norm
    with torch.no_grad():
        tokens = m.tokenizer(m._get_prompt(masked_instance_norm(data, mask)[0]), return_tensors="pt", padding=True, truncation=True,
                             max_length=512).input_ids.to(dev)
        prefix = m.llm_model.get_input_embeddings()(tokens)
    S_p, S_t, d = prefix.shape[1], m.patch_nums * C, m.d_llm
    tail = (0.02 * torch.randn(B, S_t, d, generator=g)).to(dev).requires_grad_(True)
    up_b = torch.randn(B, S_t, d, generator=g).to(dev)

    def body(fused):
        tail.grad = None
        if fused:
            out = (ops.llama_body if llama else ops.bert_body if bert else ops.gpt2_body)(m.llm_model, prefix, tail, True)
        else:
            out = m.llm_model(inputs_embeds=torch.cat([prefix, tail.to(prefix.dtype)], 1)).last_hidden_state[:, -S_t:]
        (out * up_b).sum().backward()

    def whole(fused):
        config.timellm_fused = fused
        m.zero_grad(set_to_none=True)
        (m.forecasting(tpp, data, tp, mask) * up).sum().backward()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    lines = []
    if args.prompt:
        x_norm = masked_instance_norm(data, mask)[0]

        def prompt(on):
            config.timellm_prompt_fused = on
            m._get_prompt(x_norm)

        def whole_prompt(on):
            config.timellm_prompt_fused = on
            whole(True)

        default = config.timellm_prompt_fused
        for prec in ("fp32", "bf16"):
            config.precision = prec
            line = {"tool": "timellm_bench", "leg": "prompt", "precision": prec, "B": B, "L": L, "C": C, "top_k": m.top_k, "S_p": S_p,
                    "iters": args.iters, "passes": args.passes}
            for what, fn in (("get_prompt", prompt), ("forecasting", whole_prompt)):
                for on in (True, False):
                    for _ in range(2):
                        fn(on)
                t = {True: [], False: []}
                for _ in range(args.passes):
                    for on in (True, False):
                        t[on].append(timed(lambda: fn(on), args.iters))
                for on, name in ((True, "on"), (False, "off")):
                    line[f"{what}_{name}_ms"] = round(min(t[on]), 3)
                    line[f"{what}_{name}_ms_range"] = [round(min(t[on]), 3), round(max(t[on]), 3)]
                    line[f"{what}_{name}_ms_passes"] = [round(v, 3) for v in t[on]]
                line[f"{what}_speedup"] = round(min(t[False]) / min(t[True]), 2)
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
        config.timellm_prompt_fused = default
    if args.reprogram:
        rl, E, mp = m.reprogramming_layer, m.word_embeddings, m.mapping_layer
        S, D = m.num_tokens, rl.key_projection.weight.shape[0]
        up_k, up_v = torch.randn(S, D, generator=g).to(dev), torch.randn(S, D, generator=g).to(dev)
        trainable = [mp.weight, mp.bias, rl.key_projection.weight, rl.key_projection.bias, rl.value_projection.weight, rl.value_projection.bias]

        def stage(on):
            for p_ in trainable:
                p_.grad = None
            if on:
                k, v = ops.timellm_prototypes(E, mp.weight, mp.bias, *trainable[2:], cache_on=m.llm_model)
            else:       # as models/TimeLLM.py forecasting() and ReprogrammingLayer.forward write it
                src = ops.linear(E.permute(1, 0), mp.weight, mp.bias).permute(1, 0)
                k, v = ops.linear(src, trainable[2], trainable[3]), ops.linear(src, trainable[4], trainable[5])
            torch.autograd.backward([k, v], [up_k, up_v])

        def whole_reprogram(on):
            config.timellm_reprogram_fused = on
            whole(True)

        default = config.timellm_reprogram_fused
        for prec in ("fp32", "bf16"):
            config.precision = prec
            line = {"tool": "timellm_bench", "leg": "reprogram", "precision": prec, "B": B, "S": S, "V": E.shape[0], "d_llm": d, "D": D,
                    "S_p": S_p, "iters": args.iters, "passes": args.passes, "launches_forward": 3, "launches_backward": 3}
            for what, fn in (("stage", stage), ("forecasting", whole_reprogram)):
                for on in (True, False):
                    for _ in range(2):
                        fn(on)
                t = {True: [], False: []}
                for _ in range(args.passes):
                    for on in (True, False):
                        t[on].append(timed(lambda: fn(on), args.iters))
                for on, name in ((True, "on"), (False, "off")):
                    line[f"{what}_{name}_ms"] = round(min(t[on]), 3)
                    line[f"{what}_{name}_ms_range"] = [round(min(t[on]), 3), round(max(t[on]), 3)]
                    line[f"{what}_{name}_ms_passes"] = [round(v, 3) for v in t[on]]
                line[f"{what}_speedup"] = round(min(t[False]) / min(t[True]), 2)
                line[f"{what}_every_pass_apart"] = max(t[True]) < min(t[False])
            line["reprogram_fused_calls"] = m.reprogram_fused_calls
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
        config.timellm_reprogram_fused = default
    for prec in (() if (args.prompt or args.reprogram) else ("fp32", "bf16")):
        config.precision = prec
        line = {"tool": "timellm_bench", "precision": prec, "products": args.products, "stored": args.stored, "B": B, "layers": layers, "d": d, "S_p": S_p, "S_t": S_t, "iters": args.iters,
                "passes": args.passes}
        if llama:       # the fused plan: 9 launches a layer + 3 for the last layer's tail queries + table and final norm;
            #             10 a layer backward (the attention backward is two) + the final norm's
            line.update(llm="LLAMA", launches_forward=9 * layers + 5, launches_backward=10 * layers + 1)
        if bert:        # the fused plan: 8 launches a layer + the embedding + the last layer's tail-query product and the
            #             copy that gathers its rows; backward 9 a layer in fp32 mode (the attention backward is two), 11 in bf16 mode
            #             (three, and the bf16 image of dqkv), + the embedding's and the fill of the last layer's prompt dq rows
            line.update(llm="BERT", launches_forward=8 * layers + 3, launches_backward=(11 if prec == "bf16" else 9) * layers + 2)
        for what, fn in ((("body", body),) if (llama or bert) else (("body", body), ("forecasting", whole))):
            for fused in (True, False):
                for _ in range(2):
                    fn(fused)
            t, peak = {True: [], False: []}, {True: 0.0, False: 0.0}
            for _ in range(args.passes):
                for fused in (True, False):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    t[fused].append(timed(lambda: fn(fused), args.iters))
                    peak[fused] = max(peak[fused], torch.cuda.max_memory_allocated() / 2 ** 20)
            for fused, name in ((True, "fused"), (False, "stock")):
                line[f"{what}_{name}_ms"] = round(min(t[fused]), 3)
                line[f"{what}_{name}_ms_passes"] = [round(v, 3) for v in t[fused]]
                line[f"{what}_{name}_peak_mib"] = round(peak[fused], 1)
            line[f"{what}_speedup"] = round(min(t[False]) / min(t[True]), 2)
        config.timellm_fused = True
        line["split_product_calls"] = ops.split_product_calls
        line["asplit_product_calls"] = ops.asplit_product_calls
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
