"""TTM backbone (reference models/TTM.py:11-301): the (value * mask, mask, time) rows of a window as 2C+1 series, patches of each series
lifted to d_model by one Linear, AP_levels adaptive-patching stages of e_layers TTMLayers (level i views (N, D) as (N 2^i, D / 2^i)), an
optional decoder (Linear to d_d_model, d_layers TTMLayers), and a head Linear over the flattened patches.  Same class names,
constructors, forecasting() signature and state_dict; `n_vars` and `num_patches` are written back into `configs` as the reference does.

The hot path is the layers' business (layers/MLP.py): every narrow mixer block is one HIP launch, every feature mixer three GEMMs and a
gate launch, block by block where config.ttm_fused and the limits allow; `fused_blocks` counts the blocks of the latest forecasting()
call that took a kernel.  The input build, the patcher, the head and both de-normalisations are torch around immtsf.ops.linear.

use_norm normalises TWICE, as the reference does: the adapter applies a masked instance norm to the values, shifts the mask to
mask - 0.5 and standardises the time channel (unbiased std + 1e-5); Model.forward then normalises all 2C+1 series over time again (means
detached), de-normalises all of them after the head, and the adapter de-normalises the first C."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf.ops import linear
from immtsf.dropin import fp32_entry as _fp32_entry
from layers.MLP import TTMLayer, TTMMixerBlock


class TTMAPBlock(nn.Module):
    def __init__(self, e_layers, d_model, num_patches, n_vars, mode, adapt_patch_level, dropout):
        super().__init__()
        self.adapt_patch_level = adapt_patch_level
        self.adaptive_patch_factor = 2 ** adapt_patch_level
        k = self.adaptive_patch_factor
        self.mixer_layers = nn.ModuleList([TTMLayer(d_model=d_model // k, num_patches=num_patches * k, n_vars=n_vars, mode=mode,
                                                    dropout=dropout) for _ in range(e_layers)])

    def forward(self, x):      # (B, M, N, D) -> the same shape, mixed as (B, M, N k, D / k)
        B, M, N, D = x.shape
        k = self.adaptive_patch_factor
        x = x.reshape(B, M, N * k, D // k)
        for layer in self.mixer_layers:
            x = layer(x)
        return x.reshape(B, M, x.shape[2] // k, x.shape[3] * k)


class TTMBlock(nn.Module):
    def __init__(self, e_layers, AP_levels, d_model, num_patches, n_vars, mode, dropout):
        super().__init__()
        self.AP_levels = AP_levels
        if AP_levels > 0:
            self.mixers = nn.ModuleList([TTMAPBlock(e_layers=e_layers, d_model=d_model, num_patches=num_patches, n_vars=n_vars, mode=mode,
                                                    adapt_patch_level=i, dropout=dropout) for i in reversed(range(AP_levels))])
        else:
            self.mixers = nn.ModuleList([TTMLayer(d_model=d_model, num_patches=num_patches, n_vars=n_vars, mode=mode, dropout=dropout)
                                         for _ in range(e_layers)])

    def forward(self, x):
        for m in self.mixers:
            x = m(x)
        return x


class TTMPredicationHead(nn.Module):
    def __init__(self, configs):
        super().__init__()
        self.dropout_layer = nn.Dropout(configs.dropout)
        head_d_model = configs.d_d_model if configs.use_decoder else configs.d_model
        self.base_forecast_block = nn.Linear(configs.num_patches * head_d_model, configs.pred_len)
        self.flatten = nn.Flatten(start_dim=-2)

    def forward(self, x):      # (B, M, N, D) -> (B, pred_len, M)
        x = self.dropout_layer(self.flatten(x))
        out = linear(x, self.base_forecast_block.weight, self.base_forecast_block.bias)
        return out.transpose(-1, -2).contiguous()


class TTMBackbone(nn.Module):
    def __init__(self, configs):
        super().__init__()
        self.encoder = TTMBlock(e_layers=configs.e_layers, AP_levels=configs.AP_levels, d_model=configs.d_model,
                                num_patches=configs.num_patches, n_vars=configs.n_vars, mode=configs.mode, dropout=configs.dropout)
        self.patcher = nn.Linear(configs.patch_size, configs.d_model)
        self.patch_size = configs.patch_size
        self.stride = configs.stride

    def forward(self, x):      # (B, L, M) -> (B, M, N, D); unfold drops the tail no patch covers
        x = x.permute(0, 2, 1).unfold(dimension=-1, size=self.patch_size, step=self.stride)
        return self.encoder(linear(x, self.patcher.weight, self.patcher.bias))


class Model(nn.Module):
    """forward(x, x_mark, _, y_mark) -> (B, pred_len, M), the regular-series interface of the reference"""

    def __init__(self, configs):
        super().__init__()
        configs.num_patches = (max(configs.input_len, configs.patch_size) - configs.patch_size) // configs.stride + 1
        self.configs = configs
        self.pred_len = configs.pred_len
        self.n_vars = configs.n_vars
        self.backbone = TTMBackbone(configs)
        self.use_decoder = configs.use_decoder
        self.use_norm = configs.use_norm
        if self.use_decoder:
            self.decoder_adapter = nn.Linear(configs.d_model, configs.d_d_model)
            self.decoder = TTMBlock(e_layers=configs.d_layers, AP_levels=0, d_model=configs.d_d_model, num_patches=configs.num_patches,
                                    n_vars=configs.n_vars, mode=configs.mode, dropout=configs.dropout)
        self.head = TTMPredicationHead(configs)

    def forward(self, x, x_mark, _, y_mark):
        if self.use_norm:
            means = x.mean(1, keepdim=True).detach()
            stdev = torch.sqrt(torch.var(x, dim=1, keepdim=True, unbiased=False) + 1e-5)
            x = (x - means) / stdev
        dec = self.backbone(x)
        if self.use_decoder:
            dec = self.decoder(linear(dec, self.decoder_adapter.weight, self.decoder_adapter.bias))
        y = self.head(dec)
        if self.use_norm:
            y = y * stdev + means
        return y


class TTM(Model):
    """the irregular-series adapter: (value * mask, mask, time) as 2C+1 regular series"""
    immtsf_graphable = True      # no host syncs / data-dependent shapes in forecasting()

    def __init__(self, configs):
        self.C = configs.enc_in
        configs.n_vars = configs.enc_in * 2 + 1      # as the reference: written into the caller's configs before the backbone is built
        super().__init__(configs)
        self.orig_vars = configs.enc_in
        self.input_len = configs.input_len
        self.pred_len = configs.pred_len
        self.use_norm = configs.use_norm
        self.zeros_pad = torch.zeros(configs.batch_size, max(self.input_len, self.pred_len), self.C, device=configs.device)
        self.fused_blocks = 0        # mixer blocks of the latest forecasting() call that took a HIP kernel (tests assert which path ran)

    def mixer_blocks(self):
        return [m for m in self.modules() if isinstance(m, TTMMixerBlock)]

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        B, L, C = observed_data.shape
        assert C == self.orig_vars, f"expected {self.orig_vars} channels, got {C}"
        self.fused_blocks = 0
        if L < self.input_len:
            n = self.input_len - L
            if B > self.zeros_pad.shape[0]:      # the reference pads from batch_size rows of zeros: it fails here
                raise RuntimeError(f"TTM: {B} windows of {L} < input_len {self.input_len} steps, but the padding buffer has "
                                   f"batch_size = {self.zeros_pad.shape[0]} rows")
            observed_data = torch.cat([observed_data, self.zeros_pad[:B, :n, :]], dim=1)
            observed_mask = torch.cat([observed_mask, self.zeros_pad[:B, :n, :]], dim=1)
            observed_tp = torch.cat([observed_tp, self.zeros_pad[:B, :n, 0]], dim=1)
        Lp = tp_to_predict.size(1)      # the reference pads the horizon times to pred_len and never reads them
        vals = observed_data * observed_mask
        tp_ch = observed_tp.unsqueeze(-1)
        enc_in = torch.cat([vals, observed_mask, tp_ch], dim=-1)
        if self.use_norm:
            sums = observed_mask.sum(1).clamp(min=1)
            means = vals.sum(1) / sums
            centered = vals - means.unsqueeze(1)
            stdev = torch.sqrt(((centered * observed_mask) ** 2).sum(1) / sums + 1e-5)
            tp_n = (tp_ch - tp_ch.mean(1, keepdim=True)) / (tp_ch.std(1, keepdim=True) + 1e-5)
            enc_in = torch.cat([centered / stdev.unsqueeze(1), observed_mask - 0.5, tp_n], dim=-1)
        for blk in self.mixer_blocks():
            blk.took_kernel = False
        y = Model.forward(self, enc_in, None, None, None)[..., :C]
        self.fused_blocks = sum(1 for blk in self.mixer_blocks() if blk.took_kernel)
        if self.use_norm:
            y = y * stdev.unsqueeze(1) + means.unsqueeze(1)
        return y[:, :Lp, :]


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
