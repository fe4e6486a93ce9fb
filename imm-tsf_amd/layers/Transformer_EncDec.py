"""ConvLayer, EncoderLayer / Encoder, DecoderLayer / Decoder (reference layers/Transformer_EncDec.py:6-135): post-LN blocks whose 1x1 convolutions are the
two FFN GEMMs.  The two residual joints are block calls (immtsf.ops.residual_layer_norm, ffn_block: residual add and
dropout inside the LayerNorm kernels, activation -- ReLU or GELU -- and dropout in the GEMM epilogues); widths the
row kernels do not take (d_model % 4 != 0 or > 1024) and CPU tensors (which raise inside the ops) use the op-by-op form.
The decoder has three joints: two residual_layer_norm calls behind its attentions and one ffn_block.  ConvLayer (Informer's distilling
step) is one product of the GEMM family over the three gathered taps and the row kernels of csrc/conv_distil.hip
(immtsf.ops.conv_distil); config.informer_fused = False and widths outside conv_distil_supported use the module's own torch layers (training: the batch statistics as torch reductions)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf import config
from immtsf._lib import ImmtsfError
from immtsf.ops import (SITE_LAYER_BASE, conv_distil, conv_distil_supported, ffn_block, layer_norm, linear, residual_layer_norm,
                        residual_layernorm_supported)


def _ln(norm: nn.LayerNorm, x):
    return layer_norm(x, norm.weight, norm.bias, norm.eps)


class ConvLayer(nn.Module):
    """(B, L, d) -> (B, (L + 1) // 2 + 1, d): y[t] = b + sum_k W[:, :, k] x[(t - 2 + k) mod L] for t in [0, L + 2), BatchNorm1d over the
    B (L + 2) rows, ELU, max over {2s - 1, 2s, 2s + 1}.  The submodules carry the reference's names, so the state_dict keys match
    (norm.running_mean / running_var / num_batches_tracked included)."""

    def __init__(self, c_in):
        super().__init__()
        self.downConv = nn.Conv1d(in_channels=c_in, out_channels=c_in, kernel_size=3, padding=2, padding_mode="circular")
        self.norm = nn.BatchNorm1d(c_in)
        self.activation = nn.ELU()
        self.maxPool = nn.MaxPool1d(kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        if not x.is_cuda:
            raise ImmtsfError("immtsf ops need tensors on the GPU (HIP); there is no CPU fallback")
        norm = self.norm
        if (config.informer_fused and conv_distil_supported(x.shape[-1]) and x.shape[1] >= 2 and norm.affine and norm.track_running_stats
                and norm.momentum is not None):
            return conv_distil(x, self.downConv, norm, self.training)
        x = self.downConv(x.permute(0, 2, 1))
        if not (self.training and norm.affine and norm.track_running_stats and norm.momentum is not None):
            return self.maxPool(self.activation(norm(x))).transpose(1, 2)
        # batch statistics written out (two passes over the B (L + 2) values of a channel, which may be as few as four)
        mean = x.mean((0, 2))
        var = (x - mean[None, :, None]).square().mean((0, 2))
        with torch.no_grad():
            R = x.shape[0] * x.shape[2]
            norm.running_mean.mul_(1 - norm.momentum).add_(norm.momentum * mean)
            norm.running_var.mul_(1 - norm.momentum).add_(norm.momentum * R / max(R - 1, 1) * var)
            norm.num_batches_tracked.add_(1)
        x = (x - mean[None, :, None]) * torch.rsqrt(var + norm.eps)[None, :, None] * norm.weight[None, :, None] + norm.bias[None, :, None]
        return self.maxPool(self.activation(x)).transpose(1, 2)


class EncoderLayer(nn.Module):
    def __init__(self, attention, d_model, d_ff=None, dropout=0.1, activation="relu"):
        super().__init__()
        d_ff = d_ff or 4 * d_model
        self.attention = attention
        self.conv1 = nn.Conv1d(in_channels=d_model, out_channels=d_ff, kernel_size=1)
        self.conv2 = nn.Conv1d(in_channels=d_ff, out_channels=d_model, kernel_size=1)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.activation = F.relu if activation == "relu" else F.gelu
        self._act = "relu" if activation == "relu" else "gelu"

    def forward(self, x, attn_mask=None, tau=None, delta=None):
        new_x, attn = self.attention(x, x, x, attn_mask=attn_mask, tau=tau, delta=delta)
        if x.is_cuda and residual_layernorm_supported(x.shape[-1]):
            base = SITE_LAYER_BASE + 128         # every call draws its own Philox key, so the sites can be shared by all layers
            x = residual_layer_norm(x, new_x, self.norm1, self.dropout.p, self.training, base)
            return ffn_block(x, self.conv1, self.conv2, self.norm2, self._act, self.dropout.p, self.training, base + 1), attn
        x = x + self.dropout(new_x)
        y = x = _ln(self.norm1, x)
        y = self.dropout(self.activation(linear(y, self.conv1.weight.squeeze(-1), self.conv1.bias)))
        y = self.dropout(linear(y, self.conv2.weight.squeeze(-1), self.conv2.bias))
        return _ln(self.norm2, x + y), attn


class Encoder(nn.Module):
    def __init__(self, attn_layers, conv_layers=None, norm_layer=None):
        super().__init__()
        self.attn_layers = nn.ModuleList(attn_layers)
        self.conv_layers = nn.ModuleList(conv_layers) if conv_layers is not None else None
        self.norm = norm_layer

    def forward(self, x, attn_mask=None, tau=None, delta=None):
        attns = []
        if self.conv_layers is not None:
            for i, (attn_layer, conv_layer) in enumerate(zip(self.attn_layers, self.conv_layers)):
                x, attn = attn_layer(x, attn_mask=attn_mask, tau=tau, delta=delta if i == 0 else None)
                x = conv_layer(x)
                attns.append(attn)
            x, attn = self.attn_layers[-1](x, tau=tau, delta=None)
            attns.append(attn)
        else:
            for attn_layer in self.attn_layers:
                x, attn = attn_layer(x, attn_mask=attn_mask, tau=tau, delta=delta)
                attns.append(attn)
        if self.norm is not None:
            x = _ln(self.norm, x) if isinstance(self.norm, nn.LayerNorm) else self.norm(x)
        return x, attns


class DecoderLayer(nn.Module):
    def __init__(self, self_attention, cross_attention, d_model, d_ff=None, dropout=0.1, activation="relu"):
        super().__init__()
        d_ff = d_ff or 4 * d_model
        self.self_attention = self_attention
        self.cross_attention = cross_attention
        self.conv1 = nn.Conv1d(in_channels=d_model, out_channels=d_ff, kernel_size=1)
        self.conv2 = nn.Conv1d(in_channels=d_ff, out_channels=d_model, kernel_size=1)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.norm3 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.activation = F.relu if activation == "relu" else F.gelu
        self._act = "relu" if activation == "relu" else "gelu"

    def forward(self, x, cross, x_mask=None, cross_mask=None, tau=None, delta=None):
        fused = x.is_cuda and residual_layernorm_supported(x.shape[-1])
        base = SITE_LAYER_BASE + 132           # (EncoderLayer: + 128 ..; every call draws its own Philox key)
        new_x = self.self_attention(x, x, x, attn_mask=x_mask, tau=tau, delta=None)[0]
        if fused:
            x = residual_layer_norm(x, new_x, self.norm1, self.dropout.p, self.training, base)
        else:
            x = _ln(self.norm1, x + self.dropout(new_x))
        new_x = self.cross_attention(x, cross, cross, attn_mask=cross_mask, tau=tau, delta=delta)[0]
        if fused:
            x = residual_layer_norm(x, new_x, self.norm2, self.dropout.p, self.training, base + 1)
            return ffn_block(x, self.conv1, self.conv2, self.norm3, self._act, self.dropout.p, self.training, base + 2)
        y = x = _ln(self.norm2, x + self.dropout(new_x))
        y = self.dropout(self.activation(linear(y, self.conv1.weight.squeeze(-1), self.conv1.bias)))
        y = self.dropout(linear(y, self.conv2.weight.squeeze(-1), self.conv2.bias))
        return _ln(self.norm3, x + y)


class Decoder(nn.Module):
    def __init__(self, layers, norm_layer=None, projection=None):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        self.norm = norm_layer
        self.projection = projection

    def forward(self, x, cross, x_mask=None, cross_mask=None, tau=None, delta=None):
        for layer in self.layers:
            x = layer(x, cross, x_mask=x_mask, cross_mask=cross_mask, tau=tau, delta=delta)
        if self.norm is not None:
            x = _ln(self.norm, x) if isinstance(self.norm, nn.LayerNorm) else self.norm(x)
        if self.projection is not None:
            p = self.projection
            x = linear(x, p.weight, p.bias) if isinstance(p, nn.Linear) else p(x)
        return x


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
