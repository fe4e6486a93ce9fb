"""float64 restatement of raw-text mode's Llama note embedding over the RAGGED tokens -- each note's real tokens through the pre-norm body
on their own (no padding, no attention mask, positions 0 .. L - 1), then the mean over its rows; a note of no tokens is a zero row -- and
the builders of the local tokenizer / LlamaModel directories the Llama raw-text tests load (no test names a hub model).
One thing is NOT float64: transformers' LlamaRotaryEmbedding forms the angles in fp32 (inv_freq.float() @ position.float() under a
disabled autocast) even in a .double() model, so the restatement takes fp32 angle -> fp32 cos / sin -> cast, from the model's own
inv_freq (which covers rope_type default, linear and llama3 without restating any of them).  The installed LlamaRMSNorm also casts its
row to fp32 whatever the model's dtype is; the restatement's norm is float64 by default and fp32, transformers' way, on request
(norm32) -- used only where the restatement is pinned to LlamaModel.double().
tests/test_llama_embed_ref.py pins the restatement to the padded call of the installed LlamaModel; the GPU tests compare the kernels
with it."""
import math

import torch

CORPUS = ["the patient was seen at noon", "blood pressure stable overnight", "no acute distress, plan unchanged",
          "river level rising after heavy rain", "0123456789 .,;:-"]
BOS, EOS = "<|begin_of_text|>", "<|end_of_text|>"
LLAMA3_ROPE = {"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
               "original_max_position_embeddings": 8}
DEFAULT_ROPE = {"rope_type": "default", "rope_theta": 10000.0}


def weights64(model):
    """the parameters in float64, and the rotary module's inv_freq (a non-persistent buffer: not in the state dict) kept in fp32"""
    w = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    w["rotary_emb.inv_freq"] = model.rotary_emb.inv_freq.detach().float().cpu()
    w["rotary_emb.attention_scaling"] = torch.tensor(float(model.rotary_emb.attention_scaling), dtype=torch.float32)
    return w


def _rms(x, w, eps, norm32=False):
    if norm32:      # as the installed LlamaRMSNorm takes it: the row cast to fp32, normalised there, cast back, then the gain
        h = x.float()
        return w * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)).double()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w


def rope_tables(w, L):
    """(cos, sin) (L, head_dim) float64 values of fp32 arithmetic, as LlamaRotaryEmbedding.forward forms them"""
    ang = torch.arange(L, dtype=torch.float32)[:, None] * w["rotary_emb.inv_freq"].float()[None, :]
    emb = torch.cat([ang, ang], dim=-1)
    s = w["rotary_emb.attention_scaling"].float()
    return (emb.cos() * s).double(), (emb.sin() * s).double()


def _rotate(x, cos, sin):
    half = x.shape[-1] // 2
    return x * cos + torch.cat([-x[..., half:], x[..., :half]], dim=-1) * sin


def body(w, ids, n_layer, n_head, n_kv, eps, norm32=False):
    """ids: the L > 0 token ids of ONE note -> last hidden state (L, d) float64 (after the final norm).  norm32: take every RMSNorm in
    fp32 as transformers' LlamaRMSNorm does in a model of any dtype (the pin against LlamaModel.double() needs it: see the test); the
    default is float64 throughout, which is what the kernels are measured against."""
    ids = torch.as_tensor(ids, dtype=torch.long)
    L = ids.numel()
    x = w["embed_tokens.weight"][ids]
    hd = w["layers.0.self_attn.q_proj.weight"].shape[0] // n_head
    cos, sin = rope_tables(w, L)
    causal = torch.full((L, L), float("-inf"), dtype=torch.float64).triu(1)
    for i in range(n_layer):
        p = f"layers.{i}."
        h = _rms(x, w[p + "input_layernorm.weight"], eps, norm32)
        q = (h @ w[p + "self_attn.q_proj.weight"].T).view(L, n_head, hd).transpose(0, 1)
        k = (h @ w[p + "self_attn.k_proj.weight"].T).view(L, n_kv, hd).transpose(0, 1)
        v = (h @ w[p + "self_attn.v_proj.weight"].T).view(L, n_kv, hd).transpose(0, 1)
        q, k = _rotate(q, cos, sin), _rotate(k, cos, sin)
        k, v = (t.repeat_interleave(n_head // n_kv, dim=0) for t in (k, v))          # query head h reads K/V head h // G
        prob = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd) + causal, dim=-1)
        x = x + (prob @ v).transpose(0, 1).reshape(L, n_head * hd) @ w[p + "self_attn.o_proj.weight"].T
        h = _rms(x, w[p + "post_attention_layernorm.weight"], eps, norm32)
        g = h @ w[p + "mlp.gate_proj.weight"].T
        x = x + (g * torch.sigmoid(g) * (h @ w[p + "mlp.up_proj.weight"].T)) @ w[p + "mlp.down_proj.weight"].T
    return _rms(x, w["norm.weight"], eps, norm32)


def embed_ragged(w, notes_ids, n_layer, n_head, n_kv, eps=1e-6, norm32=False):
    """notes_ids: a list of N lists of token ids -> (N, d) float64"""
    d = w["embed_tokens.weight"].shape[1]
    out = torch.zeros(len(notes_ids), d, dtype=torch.float64)
    for n, ids in enumerate(notes_ids):
        if len(ids):
            out[n] = body(w, ids, n_layer, n_head, n_kv, eps, norm32).mean(dim=0)
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
    """a byte-level BPE trained in place with NO merges (begin / end of text + 256 byte symbols: one token per ASCII character), a
    post-processor that prepends the begin-of-text token as the Llama tokenizers do, wrapped as a fast tokenizer WITHOUT a pad token
    (load_llm gives it the end-of-text token) and saved to `path`.  The empty string is 1 token; k ASCII characters are k + 1."""
    from tokenizers import ByteLevelBPETokenizer
    from tokenizers.processors import TemplateProcessing
    from transformers import PreTrainedTokenizerFast
    bpe = ByteLevelBPETokenizer()
    bpe.train_from_iterator(iter(CORPUS), vocab_size=258, min_frequency=1, special_tokens=[BOS, EOS], show_progress=False)
    bpe._tokenizer.post_processor = TemplateProcessing(single=BOS + " $A", pair=BOS + " $A " + BOS + ":1 $B:1",
                                                       special_tokens=[(BOS, bpe.token_to_id(BOS))])
    fast = PreTrainedTokenizerFast(tokenizer_object=bpe._tokenizer, bos_token=BOS, eos_token=EOS, padding_side=padding_side)
    if path is not None:
        fast.save_pretrained(path)
    return fast


def llama_config(vocab, n_layer, hidden, n_head, n_kv, inner, max_pos, head_dim=None, rope=None, **kw):
    from transformers import LlamaConfig
    return LlamaConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=n_layer, num_attention_heads=n_head, num_key_value_heads=n_kv,
                       intermediate_size=inner, max_position_embeddings=max_pos, head_dim=head_dim or hidden // n_head,
                       rope_parameters=dict(rope or LLAMA3_ROPE), bos_token_id=0, eos_token_id=1, pad_token_id=None, **kw)


def build_llama(path, vocab, n_layer, hidden, n_head, n_kv, inner, max_pos, head_dim=None, rope=None, seed=5, **kw):
    """a tiny random LlamaModel (every parameter moved off its init so that no gain is trivial), saved beside the tokenizer"""
    from transformers import LlamaModel
    torch.manual_seed(seed)
    m = LlamaModel(llama_config(vocab, n_layer, hidden, n_head, n_kv, inner, max_pos, head_dim, rope, **kw))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    m.eval()
    if path is not None:
        m.save_pretrained(path)
    return m


def build_local_llama(path, n_layer, hidden, n_head, n_kv, inner, max_pos, head_dim=None, rope=None, padding_side="right"):
    tok = build_tokenizer(path, padding_side)
    return tok, build_llama(path, len(tok), n_layer, hidden, n_head, n_kv, inner, max_pos, head_dim, rope)
