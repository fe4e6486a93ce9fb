"""Corpus-level note embedding: what the reference's compute_text_embeddings.py loops over one note per call, as a few launches.

embed_corpus tokenises every note once (the reference's tokenizer call), orders the notes by token count, cuts that order into groups
of at most `tokens_per_batch` real tokens and sends each group through fusions.load_llm's pooling -- immtsf.ops.gpt2_embed_notes,
bert_embed_notes or llama_embed_notes over the packed tokens where the fused conditions hold, the padded formulation otherwise -- then puts the rows back
in input order on the CPU. (Grouping by length costs the fused path nothing and keeps the stock path's padded batches small.)
"""
import torch


def plan_batches(token_counts, tokens_per_batch):
    """groups of note indices, shortest notes first, each holding at most tokens_per_batch tokens (a single longer note is a group of
    its own; a note of no tokens counts as one)"""
    order = sorted(range(len(token_counts)), key=lambda i: (token_counts[i], i))
    groups, cur, used = [], [], 0
    for i in order:
        cost = max(int(token_counts[i]), 1)
        if cur and used + cost > tokens_per_batch:
            groups.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += cost
    if cur:
        groups.append(cur)
    return groups


def embed_corpus(notes, tokenizer, llm_model, max_length=1024, tokens_per_batch=16384):
    """notes: list of N strings -> (N, d) fp32 on the CPU, row i the embedding fusions.load_llm.embed_notes([[notes[i]]], ...) gives"""
    from fusions import load_llm as L
    device = next(llm_model.parameters()).device
    d = L._hidden_size(llm_model)
    out = torch.zeros(len(notes), d, dtype=torch.float32)
    if not notes:
        return out
    enc = L._tokenize(list(notes), tokenizer, max_length)
    ids, attn = enc.input_ids, enc.attention_mask
    counts = attn.sum(dim=1).tolist()
    for group in plan_batches(counts, int(tokens_per_batch)):
        rows = torch.tensor(group, dtype=torch.long)
        out[rows] = L._pool_rows(llm_model, ids, attn, rows, device).detach().float().cpu()
    return out
