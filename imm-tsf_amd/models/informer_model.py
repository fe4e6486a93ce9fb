"""Informer backbone (reference models/Informer.py:15-184): two DataEmbeddings over (value, mask, time), a ProbAttention encoder with
distilling ConvLayers, a ProbAttention decoder, masked instance norm around them.  Same constructor, forecasting() signature and
state_dict keys; served under the reference's name `models.Informer` by immtsf.dropin.overlay_module (models/__init__.py) -- a file of
that name here would hide the module of a tree behind this one, which tests/test_dropin_packages.py pins.

The layers are this build's (layers/SelfAttention_Family.py, layers/Transformer_EncDec.py; config.informer_fused steers them).  What
is around them runs as TWO fused stages (immtsf.ops.informer_front / informer_tail, csrc/informer.hip): the padding, the normalisation,
the two concatenations, the decoder's zero placeholders and both embeddings in ONE launch (two backward), and decoder.norm +
decoder.projection + the de-normalisation + the slice to the horizon in ONE (two backward) -- whenever config.informer_model_fused is
on, the tensors are fp32 on the GPU, immtsf_informer_model_supported takes the shapes, c_out == C, L <= input_len, Lp <= pred_len and no
batch tensor wants a gradient; `fused_calls` counts those calls.  Anything else -- and IMMTSF_INFORMER_MODEL_FUSED=0 -- runs the
composed path: the reference's sequence on torch ops around DataEmbedding and Decoder's own norm and projection.  The stages are fp32
in bf16 mode too."""
import torch
import torch.nn as nn

from immtsf import config
from immtsf._lib import ImmtsfError
from immtsf.dropin import fp32_entry as _fp32_entry
from immtsf.ops import informer_front, informer_model_supported, informer_tail
from layers.Embed import DataEmbedding
from layers.SelfAttention_Family import AttentionLayer, ProbAttention
from layers.Transformer_EncDec import ConvLayer, Decoder, DecoderLayer, Encoder, EncoderLayer
from models._common import masked_instance_norm, pad_history


class Informer(nn.Module):
    immtsf_graphable = True      # ProbAttention draws its samples on the device: no host syncs / data-dependent shapes in forecasting()

    def __init__(self, configs):
        super().__init__()
        self.input_len = configs.input_len
        self.seq_len = configs.input_len
        self.pred_len = configs.pred_len
        self.C = configs.C
        d, H, f, p = configs.d_model, configs.n_heads, configs.factor, configs.dropout

        def attn(mask):
            return AttentionLayer(ProbAttention(mask, f, attention_dropout=p, output_attention=False), d, H)
        self.enc_embedding = DataEmbedding(2 * self.C + 1, d, configs.embed, configs.freq, p)
        self.dec_embedding = DataEmbedding(2 * self.C + 1, d, configs.embed, configs.freq, p)
        self.encoder = Encoder([EncoderLayer(attn(False), d, configs.d_ff, dropout=p, activation=configs.activation)
                                for _ in range(configs.e_layers)],
                               [ConvLayer(d) for _ in range(configs.e_layers - 1)] if configs.distil else None, norm_layer=nn.LayerNorm(d))
        self.decoder = Decoder([DecoderLayer(attn(True), attn(False), d, configs.d_ff, dropout=p, activation=configs.activation)
                                for _ in range(configs.d_layers)], norm_layer=nn.LayerNorm(d),
                               projection=nn.Linear(d, configs.c_out, bias=True))
        self.zeros_pad = torch.zeros(configs.batch_size, max(self.input_len, self.pred_len), self.C, device=configs.device)
        self.fused_calls = 0         # forecasting() calls that took the fused stages (tests assert which path ran)

    def prob_attentions(self):
        """the ProbAttention modules in call order (sample_override / last_index_sample live on them)"""
        return [m for m in self.modules() if isinstance(m, ProbAttention)]

    def _fused_ok(self, tp_to_predict, data, tp, mask):
        B, L, C = data.shape
        proj = self.decoder.projection
        return (config.informer_model_fused and B > 0 and tp_to_predict.dim() == 2 and 1 <= L <= self.input_len and
                1 <= tp_to_predict.shape[1] <= self.pred_len and proj.out_features == C and
                all(t.dtype == torch.float32 and not t.requires_grad for t in (tp_to_predict, data, tp, mask)) and
                tuple(mask.shape) == (B, L, C) and tuple(tp.shape) == (B, L) and tp_to_predict.shape[0] == B and
                informer_model_supported(self.input_len, self.pred_len, C, proj.in_features))

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        if not all(t.is_cuda for t in (tp_to_predict, observed_data, observed_tp, observed_mask)):
            raise ImmtsfError("immtsf ops need tensors on the GPU (HIP); there is no CPU fallback")
        B, L, C = observed_data.shape
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            if L < self.input_len and B > self.zeros_pad.shape[0]:      # the reference pads from batch_size rows of zeros: it fails here
                raise RuntimeError(f"Informer: {B} windows of {L} < input_len {self.input_len} steps, but the padding buffer has "
                                   f"batch_size = {self.zeros_pad.shape[0]} rows")
            self.fused_calls += 1
            ee, de = self.enc_embedding, self.dec_embedding
            enc, dec, means, stdev = informer_front(observed_data, observed_mask, observed_tp, tp_to_predict, self.input_len, self.pred_len,
                                                    ee.value_embedding.tokenConv.weight, de.value_embedding.tokenConv.weight,
                                                    ee.position_embedding.pe, de.position_embedding.pe, ee.dropout.p, self.training)
            enc, _ = self.encoder(enc, attn_mask=None)
            for layer in self.decoder.layers:
                dec = layer(dec, enc, x_mask=None, cross_mask=None)
            return informer_tail(dec, self.decoder.norm, self.decoder.projection, means, stdev, tp_to_predict.shape[1])
        tp_to_predict, observed_data, observed_tp, observed_mask, Lp = pad_history(
            self.zeros_pad, self.input_len, self.pred_len, tp_to_predict, observed_data, observed_tp, observed_mask)
        x, means, stdev = masked_instance_norm(observed_data, observed_mask)
        zp = observed_data.new_zeros(B, self.pred_len, C)
        enc = self.enc_embedding(torch.cat([x, observed_mask, observed_tp.unsqueeze(-1)], dim=-1), None)
        dec = self.dec_embedding(torch.cat([zp, zp, tp_to_predict.unsqueeze(-1)], dim=-1), None)
        enc, _ = self.encoder(enc, attn_mask=None)
        dec = self.decoder(dec, enc, x_mask=None, cross_mask=None)
        return (dec * stdev + means)[:, :Lp, :]


def install(module):
    """`module` is the models/Informer.py of a tree behind this one, just executed (immtsf/dropin.py, overlay_module): when what it
    defines as `Informer` is the reference's model -- an nn.Module subclass with a forecasting() -- this build's class takes its place;
    anything else under that name is left alone"""
    theirs = getattr(module, "Informer", None)
    if isinstance(theirs, type) and issubclass(theirs, nn.Module) and callable(getattr(theirs, "forecasting", None)):
        module.Informer = Informer
