"""Fixtures' options, an Informer-shaped stack of the product's layers, error measures and seeded tensors shared by
tests/test_informer_ref.py, tests/test_informer_dropin.py (CPU) and tests/test_gpu_informer.py (GPU).  The product ships no
models/Informer.py (the reference's own file runs on these layers); `Stack` composes them the same way, for the tests."""
import os
import types

import numpy as np
import torch
import torch.nn as nn

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2      # the project's fp32 bars (ttm_cases.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_COMMON = dict(C=3, c_out=3, input_len=12, pred_len=5, d_model=16, d_ff=32, d_layers=1, embed="fixed", freq="h")
FIXTURES = {
    "model_informer": dict(_COMMON, n_heads=2, e_layers=2, factor=1, distil=True, activation="gelu"),
    "model_informer_nodistil": dict(_COMMON, n_heads=4, e_layers=3, factor=3, distil=False, activation="relu"),
}
CONV_CASES = {"a": (1, 2, 4), "b": (3, 9, 8)}


def config(opts, batch_size=4, device="cpu", dropout=0.0, **over):
    cfg = types.SimpleNamespace(batch_size=batch_size, device=device, dropout=dropout, **opts)
    cfg.__dict__.update(over)
    return cfg


class Stack(nn.Module):
    """the composition of models/Informer.py from the product's layers: same submodule names, so the same state_dict keys"""

    def __init__(self, cfg):
        super().__init__()
        from layers.Embed import DataEmbedding
        from layers.SelfAttention_Family import AttentionLayer, ProbAttention
        from layers.Transformer_EncDec import ConvLayer, Decoder, DecoderLayer, Encoder, EncoderLayer
        self.cfg = cfg
        d, H, f, p = cfg.d_model, cfg.n_heads, cfg.factor, cfg.dropout

        def attn(mask):
            return AttentionLayer(ProbAttention(mask, f, attention_dropout=p, output_attention=False), d, H)
        self.enc_embedding = DataEmbedding(2 * cfg.C + 1, d, cfg.embed, cfg.freq, p)
        self.dec_embedding = DataEmbedding(2 * cfg.C + 1, d, cfg.embed, cfg.freq, p)
        self.encoder = Encoder([EncoderLayer(attn(False), d, cfg.d_ff, dropout=p, activation=cfg.activation) for _ in range(cfg.e_layers)],
                               [ConvLayer(d) for _ in range(cfg.e_layers - 1)] if cfg.distil else None, norm_layer=nn.LayerNorm(d))
        self.decoder = Decoder([DecoderLayer(attn(True), attn(False), d, cfg.d_ff, dropout=p, activation=cfg.activation)
                                for _ in range(cfg.d_layers)], norm_layer=nn.LayerNorm(d), projection=nn.Linear(d, cfg.c_out, bias=True))

    def prob_attentions(self):
        """the ProbAttention modules in call order"""
        from layers.SelfAttention_Family import ProbAttention
        return [m for m in self.modules() if isinstance(m, ProbAttention)]

    def forecasting(self, tpp, data, tp, mask):
        cfg = self.cfg
        B, L, C = data.shape
        if L < cfg.input_len:
            z = data.new_zeros(B, cfg.input_len - L, C)
            data, mask, tp = torch.cat([data, z], 1), torch.cat([mask, z], 1), torch.cat([tp, z[:, :, 0]], 1)
        Lp = tpp.shape[1]
        if Lp < cfg.pred_len:
            tpp = torch.cat([tpp, tpp.new_zeros(B, cfg.pred_len - Lp)], 1)
        cnt = mask.sum(1, keepdim=True).clamp(min=1)
        x = data * mask
        means = x.sum(1, keepdim=True) / cnt
        x = x - means
        stdev = torch.sqrt(((x * mask) ** 2).sum(1, keepdim=True) / cnt + 1e-5)
        x = x / stdev
        zp = data.new_zeros(B, cfg.pred_len, C)
        enc = self.enc_embedding(torch.cat([x, mask, tp.unsqueeze(-1)], -1), None)
        dec = self.dec_embedding(torch.cat([zp, zp, tpp.unsqueeze(-1)], -1), None)
        enc, _ = self.encoder(enc, attn_mask=None)
        dec = self.decoder(dec, enc, x_mask=None, cross_mask=None)
        return (dec * stdev + means)[:, :Lp]


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    none = {s for s in str(z["none"]).split("\n") if s}
    samples = [torch.from_numpy(z[f"sample.{i}"]) for i in range(len([k for k in z.files if k.startswith("sample.")]))]
    return z, params, none, samples


def golden_model(name, dev, **over):
    """the Stack with the fixture's state, in train mode on `dev`; -> (module, (tpp, data, tp, mask, upstream), golden)"""
    z, params, none, samples = golden(name)
    m = Stack(config(FIXTURES[name], device=str(dev), **over))
    m.load_state_dict(params, strict=True)
    m = m.to(dev).train()
    batch = tuple(torch.from_numpy(z[k]).to(dev) for k in ("tpp", "data", "tp", "mask", "upstream"))
    return m, batch, (z, params, none, samples)


def rel(a, b, floor=1e-3):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def grad_errors(got, want):
    """got / want: name -> gradient or None.  -> (the names whose None-ness differs, name -> error relative to max(|want|, 1e-2 of the
    largest gradient))"""
    gmax = max(float(w.abs().max()) for w in want.values() if w is not None)
    diff = sorted(k for k in want if (want[k] is None) != (got[k] is None))
    return diff, {k: rel(got[k], w, floor=GRAD_FLOOR * gmax) for k, w in want.items() if w is not None and got[k] is not None}


def conv_params(z, case):
    """name -> tensor of ConvLayer fixture `case` (state before the calls)"""
    pre = f"{case}.p."
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
