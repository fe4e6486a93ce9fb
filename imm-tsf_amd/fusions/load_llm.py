"""The text side's front door: hidden sizes of the LLMs whose note embeddings feed the fusion blocks, and raw-text mode.

get_d_model / get_context_window_size mirror the alias table of the reference's fusions/load_llm.py:5-13 as local lookups (the
reference asks the HF hub, which needs network access; the fusion constructors only need the integers).

load_llm / embed_notes (reference :79-201) keep the reference's signatures and results.  embed_notes pads every note to max_length
tokens, runs the padded batch through the frozen LLM and averages each note's real-token rows.  For a GPT2Model, a BertModel or a
LlamaModel (Llama-3.1, deepseek-llm) on the GPU behind a right-padding tokenizer the same function is computed over the real tokens alone
(immtsf.ops.gpt2_embed_notes, llama_embed_notes: a causal model never lets a pad token into a real token's hidden state, and Llama's
rotary positions are arange(seq) whatever the mask is; immtsf.ops.bert_embed_notes: a padded key has an exact zero weight in a real
query's softmax; the average never reads a pad row), so only the real ids are uploaded.  The padded-out notes of a window are the empty
string: where that has no tokens (GPT-2) their rows are zeros without being run, where it has some (BERT's [CLS] [SEP], Llama's BOS) the
one note is run once in the same call and copied to every such row.  A Llama whose parameters are all stored in bf16 (what load_llm
returns for the Llama / DeepSeek aliases: their checkpoints are bf16 and from_pretrained keeps the stored dtype) takes the same path with
immtsf.config.llama_stored_bf16 on, its weights read in place, and the pooled rows come back in bf16 as the padded call returns them.
Every other case -- another model class, a Llama outside llama_embed_notes_supported (parameters stored in bf16 with that knob off, fp16
or mixed dtypes, dynamic / yarn / longrope RoPE), a left-padding tokenizer, the CPU, immtsf.config.note_embed_fused off, a model left in
training mode with dropout -- runs the padded formulation on torch ops.
path_calls counts which way each call went.
"""
import torch

from immtsf import config

_D_MODEL = {
    "GPT2": 768, "GPT2M": 1024, "GPT2L": 1280, "GPT2XL": 1600, "BERT": 768, "Llama": 4096, "DeepSeek": 4096,
    "openai-community/gpt2": 768, "openai-community/gpt2-medium": 1024, "openai-community/gpt2-large": 1280,
    "openai-community/gpt2-xl": 1600, "google-bert/bert-base-uncased": 768, "meta-llama/Llama-3.1-8B": 4096,
    "deepseek-ai/deepseek-llm-7b-base": 4096,
}


def register_d_model(name: str, d_model: int) -> None:
    """Teach the table a new alias (tests use small toy widths)."""
    _D_MODEL[name] = int(d_model)


def get_d_model(llm_model_fusion: str) -> int:
    try:
        return _D_MODEL[llm_model_fusion]
    except KeyError:
        raise KeyError(
            f"unknown LLM alias {llm_model_fusion!r}: add it with fusions.load_llm.register_d_model(name, d_model)") from None


_CONTEXT = {"GPT2": 1024, "GPT2M": 1024, "GPT2L": 1024, "GPT2XL": 1024, "BERT": 512, "Llama": 131072, "DeepSeek": 4096,
            "openai-community/gpt2": 1024, "openai-community/gpt2-medium": 1024, "openai-community/gpt2-large": 1024,
            "openai-community/gpt2-xl": 1024, "google-bert/bert-base-uncased": 512, "meta-llama/Llama-3.1-8B": 131072,
            "deepseek-ai/deepseek-llm-7b-base": 4096}


def get_context_window_size(llm_model_fusion: str, device="cpu") -> int:
    """positional context window of the LLM (reference :38-76 loads the model to read it; a table here, same values
    as the alias comments at :5-13)"""
    try:
        return _CONTEXT[llm_model_fusion]
    except KeyError:
        raise KeyError(f"unknown LLM alias {llm_model_fusion!r}") from None


_HUB_ID = {"GPT2": "openai-community/gpt2", "GPT2M": "openai-community/gpt2-medium", "GPT2L": "openai-community/gpt2-large",
           "GPT2XL": "openai-community/gpt2-xl", "BERT": "google-bert/bert-base-uncased", "Llama": "meta-llama/Llama-3.1-8B",
           "DeepSeek": "deepseek-ai/deepseek-llm-7b-base"}

path_calls = {"fused": 0, "stock": 0}      # embed_notes / embed_notes_packed calls by the path that computed them


def load_llm(llm_model_fusion: str, llm_layers_fusion: int | None = None, device="cpu", use_device_map: bool = False):
    """(tokenizer, frozen model) of an alias of the table above, a hub id or a local directory (anything that is not an alias goes to
    from_pretrained untouched).  A tokenizer without a pad token pads with eos; llm_layers_fusion cuts the layer stack only where the
    model has `encoder.layer` (BERT-like: a GPT-2 keeps all its blocks, as in the reference); the embedding table is resized to the
    tokenizer's length."""
    from transformers import AutoModel, AutoTokenizer
    source = _HUB_ID.get(llm_model_fusion, llm_model_fusion)
    tokenizer = AutoTokenizer.from_pretrained(source)
    if tokenizer.pad_token is None:
        tokenizer.pad_token = tokenizer.eos_token
        tokenizer.pad_token_id = tokenizer.eos_token_id
    if use_device_map:
        llm_model = AutoModel.from_pretrained(source, device_map="auto")
    else:
        llm_model = AutoModel.from_pretrained(source).to(device)
    stack = getattr(getattr(llm_model, "encoder", None), "layer", None)
    if llm_layers_fusion is not None and stack is not None:
        llm_model.encoder.layer = torch.nn.ModuleList(list(stack)[:llm_layers_fusion])
    llm_model.requires_grad_(False)
    llm_model.resize_token_embeddings(len(tokenizer))
    return tokenizer, llm_model


def _tokenize(texts, tokenizer, max_length):
    return tokenizer(texts, padding="max_length", truncation=True, max_length=max_length, return_tensors="pt")


def _token_counts(attn):
    """(per-row token counts, whether every row of the 0 / 1 mask is a right-padded prefix) on the host"""
    counts = attn.sum(dim=1)
    prefix = torch.arange(attn.shape[1]).unsqueeze(0) < counts.unsqueeze(1)
    return counts, bool(torch.equal(prefix, attn.bool()))


def _family(llm_model):
    """what the fused path needs to know of a model family: (the packed-token op, its limits, the fewest notes of an fp32 call that take
    it, the config's dropout rates), or None for a model without one"""
    from transformers import BertModel, GPT2Model, LlamaModel

    from immtsf import ops
    if isinstance(llm_model, GPT2Model):
        return (ops.gpt2_embed_notes, ops.gpt2_embed_notes_supported, config.note_embed_fp32_min_notes,
                ("embd_pdrop", "attn_pdrop", "resid_pdrop"))
    if type(llm_model) is BertModel:
        return (ops.bert_embed_notes, ops.bert_embed_notes_supported, config.bert_embed_fp32_min_notes,
                ("hidden_dropout_prob", "attention_probs_dropout_prob"))
    if type(llm_model) is LlamaModel:
        return (ops.llama_embed_notes, ops.llama_embed_notes_supported, config.llama_embed_fp32_min_notes, ("attention_dropout",))
    return None


def _fused_ok(llm_model, device, max_length, n_notes):
    if not config.note_embed_fused or device.type != "cuda":
        return False
    family = _family(llm_model)
    if family is None:
        return False
    _, supported, fp32_min_notes, drops = family
    if config.precision_code(None) == 0 and n_notes < fp32_min_notes:
        return False             # (measured slower than the padded call there: DESIGN 4o, 4p, 4q)
    if not supported(llm_model, max_length):
        return False
    cfg = llm_model.config       # (a body left in training mode draws dropout masks in the padded formulation: that is not this kernel)
    return not (llm_model.training and max(float(getattr(cfg, k)) for k in drops) > 0.0)


def _pool_padded(llm_model, ids, attn):
    """the reference's formulation (:188-195): the padded batch through the model, mean over the rows the mask keeps"""
    hidden = llm_model(input_ids=ids, attention_mask=attn).last_hidden_state
    keep = attn.unsqueeze(-1)
    return (hidden * keep).sum(dim=1) / keep.sum(dim=1).clamp(min=1)


def _pool_rows(llm_model, ids, attn, rows, device):
    """pooled embeddings (len(rows), d) of the tokenised rows `rows` (host index tensor) of ids / attn, on `device`"""
    ids, attn = ids[rows], attn[rows]
    counts, is_prefix = _token_counts(attn)
    if is_prefix and rows.numel() and _fused_ok(llm_model, device, int(ids.shape[1]), int(rows.numel())):
        real = ids[attn.bool()]                       # row-major: the notes' real tokens back to back
        if real.numel() and (int(real.min()) < 0 or int(real.max()) >= llm_model.get_input_embeddings().weight.shape[0]):
            raise IndexError("embed_notes: a token id lies outside the model's embedding table")
        cu = torch.zeros(rows.numel() + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(counts, 0)
        path_calls["fused"] += 1
        emb = _family(llm_model)[0](llm_model, real.to(torch.int32).to(device), cu.to(device), max_len=max(int(counts.max()), 1))
        stored = next(llm_model.parameters()).dtype       # (the padded call returns the model's dtype: so does this one)
        return emb if stored == torch.float32 else emb.to(stored)
    path_calls["stock"] += 1
    return _pool_padded(llm_model, ids.to(device), attn.to(device))


def _hidden_size(llm_model):
    cfg = llm_model.config
    return int(getattr(cfg, "hidden_size", None) or cfg.n_embd)


def embed_notes(notes_text: list[list[str]], tokenizer, llm_model, max_length: int = 1024):
    """notes_text: B windows, each a list of strings -> (embeddings (B, N_max, d), note mask (B, N_max) bool: True where the window has
    a note) on the model's device.  Reference :130-201."""
    device = next(llm_model.parameters()).device
    B = len(notes_text)
    per_window = [len(w) for w in notes_text]
    N_max = max(per_window, default=0)
    note_mask = torch.arange(N_max).unsqueeze(0) < torch.tensor(per_window, dtype=torch.long).view(B, 1)
    if B * N_max == 0:
        return torch.zeros(B, N_max, _hidden_size(llm_model), device=device), note_mask.to(device)
    enc = _tokenize([n for w in notes_text for n in list(w) + [""] * (N_max - len(w))], tokenizer, max_length)
    ids, attn = enc.input_ids, enc.attention_mask
    every = torch.arange(B * N_max)
    real, fill = every[note_mask.reshape(-1)], every[~note_mask.reshape(-1)]
    # the padded-out notes are all the empty string: run one of them when it has tokens ([CLS] [SEP]); none when it has not (zero rows)
    one_fill = fill[:1] if fill.numel() and int(attn[fill[0]].sum()) > 0 else fill[:0]
    run = torch.cat([real, one_fill])
    counts, is_prefix = _token_counts(attn[run])
    if is_prefix and run.numel() and _fused_ok(llm_model, device, int(ids.shape[1]), int(run.numel())):
        emb = _pool_rows(llm_model, ids, attn, run, device)
        out = torch.zeros(B * N_max, _hidden_size(llm_model), device=device, dtype=emb.dtype)
        out[real.to(device)] = emb[:real.numel()]
        if one_fill.numel():
            out[fill.to(device)] = emb[-1]
    else:                  # every row, the padded-out notes included, as the reference runs them
        out = _pool_rows(llm_model, ids, attn, every, device)
    return out.view(B, N_max, -1), note_mask.to(device)


def embed_notes_packed(notes_text: list[list[str]], tokenizer, llm_model, max_length: int = 1024):
    """embed_notes without the padded (B, N_max, d) tensor: (embeddings (sum N, d) of the windows' notes back to back, notes per window
    (B) int32, N_max) -- what immtsf.ops.PackedNotes takes.  Only the windows' own notes are tokenised and run."""
    device = next(llm_model.parameters()).device
    per_window = [len(w) for w in notes_text]
    lengths = torch.tensor(per_window, dtype=torch.int32).to(device)
    flat = [n for w in notes_text for n in w]
    if not flat:
        return torch.zeros(0, _hidden_size(llm_model), device=device), lengths, 0
    enc = _tokenize(flat, tokenizer, max_length)
    emb = _pool_rows(llm_model, enc.input_ids, enc.attention_mask, torch.arange(len(flat)), device)
    return emb, lengths, max(per_window)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
