"""float64 restatement of raw-text mode's BERT note embedding over the RAGGED tokens -- each note's real tokens through the post-LN body on
their own (no padding, no attention mask, token type 0), then the mean over its rows; a note of no tokens is a zero row -- and the
builders of the local WordPiece tokenizer / BertModel directories the BERT raw-text tests load (no test names a hub model).
tests/test_bert_embed_ref.py pins the restatement to the padded call of the installed BertModel; the GPU tests compare the kernels
with it."""
import math

import torch

CORPUS = ["the patient was seen at noon", "blood pressure stable overnight", "no acute distress , plan unchanged",
          "river level rising after heavy rain", "a b c d e f g h i j k l m n o p q r s t u v w x y z"]
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]


def weights64(model):
    return {k: v.detach().double().cpu() for k, v in model.state_dict().items()}


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _lin(x, w, name):
    return x @ w[name + ".weight"].T + w[name + ".bias"]


def body(w, ids, n_layer, n_head, eps):
    """ids: the L > 0 token ids of ONE note -> last hidden state (L, d) float64"""
    ids = torch.as_tensor(ids, dtype=torch.long)
    L = ids.numel()
    e = "embeddings."
    x = w[e + "word_embeddings.weight"][ids] + w[e + "position_embeddings.weight"][:L] + w[e + "token_type_embeddings.weight"][0]
    x = _ln(x, w[e + "LayerNorm.weight"], w[e + "LayerNorm.bias"], eps)
    d = x.shape[1]
    hd = d // n_head
    for i in range(n_layer):
        p = f"encoder.layer.{i}."
        q, k, v = (_lin(x, w, p + "attention.self." + n).view(L, n_head, hd).transpose(0, 1) for n in ("query", "key", "value"))
        prob = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), dim=-1)          # (H, L, L): every query sees every key of the note
        ctx = (prob @ v).transpose(0, 1).reshape(L, d)
        x = _ln(_lin(ctx, w, p + "attention.output.dense") + x, w[p + "attention.output.LayerNorm.weight"],
                w[p + "attention.output.LayerNorm.bias"], eps)
        h = _lin(x, w, p + "intermediate.dense")
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = _ln(_lin(h, w, p + "output.dense") + x, w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"], eps)
    return x


def embed_ragged(w, notes_ids, n_layer, n_head, eps=1e-12):
    """notes_ids: a list of N lists of token ids -> (N, d) float64"""
    d = w["embeddings.word_embeddings.weight"].shape[1]
    out = torch.zeros(len(notes_ids), d, dtype=torch.float64)
    for n, ids in enumerate(notes_ids):
        if len(ids):
            out[n] = body(w, ids, n_layer, n_head, eps).mean(dim=0)
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


def build_wordpiece_tokenizer(path, padding_side="right"):
    """a WordPiece trained in place on a few lines, with BERT's [CLS] $A [SEP] post-processor, wrapped as a fast tokenizer with
    [PAD] / [UNK] / [CLS] / [SEP] / [MASK] and saved to `path`.  The empty string is 2 tokens; k space-separated letters are k + 2.
    The trainer breaks ties between equally frequent pairs in hash order, which differs from process to process, so it is asked for no
    merges (the vocabulary is the corpus's characters and their ## forms: one token per character, as the GPT-2 stand-in) and the ids
    are dealt again in sorted order: every process builds the tokenizer the golden was written with."""
    from tokenizers import BertWordPieceTokenizer
    from tokenizers.processors import TemplateProcessing
    from transformers import PreTrainedTokenizerFast
    wp = BertWordPieceTokenizer(lowercase=True)
    wp.train_from_iterator(iter(CORPUS), vocab_size=len(SPECIALS), min_frequency=1, special_tokens=SPECIALS, show_progress=False)
    pieces = SPECIALS + sorted(t for t in wp.get_vocab() if t not in SPECIALS)
    wp = BertWordPieceTokenizer(vocab={t: i for i, t in enumerate(pieces)}, lowercase=True)
    wp._tokenizer.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                      special_tokens=[("[CLS]", wp.token_to_id("[CLS]")), ("[SEP]", wp.token_to_id("[SEP]"))])
    fast = PreTrainedTokenizerFast(tokenizer_object=wp._tokenizer, pad_token="[PAD]", unk_token="[UNK]", cls_token="[CLS]", sep_token="[SEP]",
                                   mask_token="[MASK]", padding_side=padding_side)
    if path is not None:
        fast.save_pretrained(path)
    return fast


def bert_config(vocab, n_layer, hidden, n_head, inner, max_pos, **kw):
    from transformers import BertConfig
    return BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=n_layer, num_attention_heads=n_head, intermediate_size=inner,
                      max_position_embeddings=max_pos, pad_token_id=0, **kw)


def build_bert(path, vocab, n_layer, hidden, n_head, inner, max_pos, seed=5, **kw):
    """a tiny random BertModel (every parameter moved off its init so that no bias or gain is trivial), saved beside the tokenizer"""
    from transformers import BertModel
    torch.manual_seed(seed)
    m = BertModel(bert_config(vocab, n_layer, hidden, n_head, inner, max_pos, **kw))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    m.eval()
    if path is not None:
        m.save_pretrained(path)
    return m


def build_local_bert(path, n_layer, hidden, n_head, inner, max_pos, padding_side="right"):
    tok = build_wordpiece_tokenizer(path, padding_side)
    return tok, build_bert(path, len(tok), n_layer, hidden, n_head, inner, max_pos)
