"""TimeMixer backbone (reference models/TimeMixer.py:9-326): masked instance norm, (value, mask, time) rows, a pyramid of down-sampled
copies, one DataEmbedding per scale, e_layers past-decomposable-mixing blocks (decomposition, bottom-up season mixing, top-down trend
mixing, a feature MLP with residual), a Linear over time on the COARSEST scale, the projection to C channels, de-normalisation.  Same
class names, signature and state_dict; the clipped `down_sampling_layers` is written back into `configs` as the reference does.

forecasting() is ONE HIP launch (immtsf.ops.timemixer_forecast, csrc/timemixer.hip) and its backward TWO (parameter gradients only,
summed in a fixed order) whenever config.timemixer_fused is on, the options are the reference's defaults (moving_avg decomposition
with an odd window, channel independence, average pooling, window 2), the tensors are fp32 on the GPU, immtsf_timemixer_supported takes
the shapes and neither data, mask nor times wants a gradient; `fused_calls` counts those calls.  Anything else -- and
IMMTSF_TIMEMIXER_FUSED=0 -- runs the composed path below, which covers every option: one token_embed kernel per scale, torch
element-wise ops and pooling around immtsf.ops.linear calls (one HIP GEMM each).  The fused path is fp32 in bf16 mode too.

Only the coarsest scale reaches the output (predict_layers[-1] on enc_out_list[-1]), so in the LAST block the trend mixing and the
out_layer results of the finer scales have no reader: both paths skip them, and the parameters without a gradient are the reference's
(normalize_layers.*, the temporal embedding, predict_layers[0 .. n-1], the last block's mix_trend.*)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf import config
from immtsf.ops import linear, timemixer_forecast, timemixer_params, timemixer_supported
from immtsf.dropin import fp32_entry as _fp32_entry
from layers.Autoformer_EncDec import series_decomp
from layers.Embed import DataEmbedding
from layers.StandardNorm import Normalize
from models._common import masked_instance_norm


def _mlp(seq, x):
    """nn.Sequential(Linear, GELU, Linear) on the last axis: two HIP GEMMs around the exact (erf) GELU"""
    return linear(F.gelu(linear(x, seq[0].weight, seq[0].bias)), seq[2].weight, seq[2].bias)


def _mixer(a, b):
    return nn.Sequential(nn.Linear(a, b), nn.GELU(), nn.Linear(b, b))


class DFT_series_decomp(nn.Module):
    """season = the top_k strongest frequencies (the mean excluded) of each feature over time, trend = the rest"""

    def __init__(self, top_k=5):
        super().__init__()
        self.top_k = top_k

    def forward(self, x):                       # (B, T, d)
        xf = torch.fft.rfft(x, dim=1)
        freq = xf.abs()
        freq[:, 0, :] = 0
        cutoff = torch.topk(freq, self.top_k, dim=1)[0].min(dim=1, keepdim=True)[0]
        xf[freq <= cutoff] = 0
        season = torch.fft.irfft(xf, n=x.size(1), dim=1)
        return season, x - season


class MultiScaleSeasonMixing(nn.Module):
    """bottom-up: scale i+1 takes Linear(T_i -> T_{i+1}) GELU Linear(T_{i+1} -> T_{i+1}) of the mixed scale i"""

    def __init__(self, configs):
        super().__init__()
        S, w = configs.input_len, configs.down_sampling_window
        self.down_sampling_layers = nn.ModuleList([_mixer(S // w ** i, S // w ** (i + 1)) for i in range(configs.down_sampling_layers)])

    def forward(self, season_list, coarsest_only=False):      # each (B, d, T_i) -> each (B, T_i, d)
        high, low = season_list[0], season_list[1]            # one scale alone: the reference's IndexError
        out = [high]
        for i, layer in enumerate(self.down_sampling_layers):
            high = low + _mlp(layer, high)
            if i + 2 < len(season_list):
                low = season_list[i + 2]
            out.append(high)
        return [o.permute(0, 2, 1) for o in (out[-1:] if coarsest_only else out)]


class MultiScaleTrendMixing(nn.Module):
    """top-down: up_sampling_layers[m] lifts the mixed scale n-m to scale n-1-m"""

    def __init__(self, configs):
        super().__init__()
        S, w = configs.input_len, configs.down_sampling_window
        self.up_sampling_layers = nn.ModuleList([_mixer(S // w ** (i + 1), S // w ** i)
                                                 for i in reversed(range(configs.down_sampling_layers))])

    def forward(self, trend_list):
        rev = list(reversed(trend_list))
        low, high = rev[0], rev[1]
        out = [low]
        for i, layer in enumerate(self.up_sampling_layers):
            low = high + _mlp(layer, low)
            if i + 2 < len(rev):
                high = rev[i + 2]
            out.append(low)
        return [o.permute(0, 2, 1) for o in reversed(out)]


class PastDecomposableMixing(nn.Module):
    def __init__(self, configs):
        super().__init__()
        self.seq_len = configs.input_len
        self.pred_len = configs.pred_len
        self.down_w = configs.down_sampling_window
        self.decomposition = series_decomp(configs.moving_avg) if configs.decomp_method == "moving_avg" else \
            DFT_series_decomp(configs.top_k)
        if not configs.channel_independence:
            self.cross_layer = nn.Sequential(nn.Linear(configs.d_model, configs.d_ff), nn.GELU(), nn.Linear(configs.d_ff, configs.d_model))
        self.mix_season = MultiScaleSeasonMixing(configs)
        self.mix_trend = MultiScaleTrendMixing(configs)
        self.out_layer = nn.Sequential(nn.Linear(configs.d_model, configs.d_ff), nn.GELU(), nn.Linear(configs.d_ff, configs.d_model))

    def forward(self, x_list, last=False):
        """x_list: (B, T_i, d) per scale.  last: only the coarsest result has a reader -- the trend mixing (its coarsest output is
        its coarsest input) and the finer scales' out_layer are skipped, and the list comes back with the coarsest entry replaced."""
        seasons, trends = [], []
        for x in x_list:
            s, t = self.decomposition(x)
            if hasattr(self, "cross_layer"):
                s, t = _mlp(self.cross_layer, s), _mlp(self.cross_layer, t)
            seasons.append(s.permute(0, 2, 1))
            trends.append(t.permute(0, 2, 1))
        if last:
            os_ = self.mix_season(seasons, coarsest_only=True)[0]
            return x_list[:-1] + [x_list[-1] + _mlp(self.out_layer, os_ + trends[-1].permute(0, 2, 1))]
        out_seasons, out_trends = self.mix_season(seasons), self.mix_trend(trends)
        return [x + _mlp(self.out_layer, s + t) for x, s, t in zip(x_list, out_seasons, out_trends)]


class TimeMixer(nn.Module):
    immtsf_graphable = True      # no host syncs / data-dependent shapes in forecasting()

    def __init__(self, configs):
        super().__init__()
        self.input_len = configs.input_len
        self.pred_len = configs.pred_len
        self.C = configs.enc_in
        self.layers = configs.e_layers
        n, cur = 0, configs.input_len
        while n < configs.down_sampling_layers and cur >= configs.down_sampling_window:
            cur //= configs.down_sampling_window
            n += 1
        configs.down_sampling_layers = n      # as the reference: the clipped count goes back into the caller's configs
        self.down_layers = n
        self.down_w = configs.down_sampling_window
        self.configs = configs
        self.zeros_pad = torch.zeros(configs.batch_size, max(self.input_len, self.pred_len), self.C, device=configs.device)
        self.enc_embedding = DataEmbedding(2 * self.C + 1, configs.d_model, configs.embed, configs.freq, configs.dropout)
        self.normalize_layers = nn.ModuleList([Normalize(self.C, affine=True, non_norm=False) for _ in range(n + 1)])
        self.predict_layers = nn.ModuleList([nn.Linear(configs.input_len // self.down_w ** i, configs.pred_len) for i in range(n + 1)])
        self.projection = nn.Linear(configs.d_model, self.C, bias=True)
        self.pdm_blocks = nn.ModuleList([PastDecomposableMixing(configs) for _ in range(self.layers)])
        self.fused_calls = 0         # forecasting() calls that took the fused HIP path (tests assert which path ran)
        self._last_drop = None       # (p, seed, site, counter pointer) of the latest fused call's dropout

    def _multi_scale(self, x_enc):
        """x_enc (B, T, 2C+1) -> the pyramid.  The reference also down-samples the mask (m_list) and never reads it."""
        method, w = self.configs.down_sampling_method, self.down_w
        if method == "max":
            pool = nn.MaxPool1d(w)
        elif method == "avg":
            pool = nn.AvgPool1d(w)
        elif method == "conv":      # as the reference: a fresh, randomly initialised convolution on the CPU in every call
            pool = nn.Conv1d(in_channels=x_enc.size(-1), out_channels=x_enc.size(-1), kernel_size=3, padding=1, stride=w,
                             padding_mode="circular", bias=False)
        else:
            return [x_enc]
        cur = x_enc.permute(0, 2, 1)
        xs = [x_enc]
        for _ in range(self.down_layers):
            cur = pool(cur)
            if cur.size(-1) == 0:
                break
            xs.append(cur.permute(0, 2, 1))
        return xs

    def _fused_dims(self):
        c = self.configs
        if not (c.decomp_method == "moving_avg" and c.channel_independence == 1 and c.down_sampling_method == "avg" and
                self.down_w == 2):
            return None
        return (self.input_len, self.pred_len, self.C, int(c.d_model), int(c.d_ff), self.layers, self.down_layers, int(c.moving_avg))

    def _fused_ok(self, tp_to_predict, data, tp, mask):
        B, L, C = data.shape
        dims = self._fused_dims()
        if not (config.timemixer_fused and dims is not None and B > 0 and L <= self.input_len and
                tp_to_predict.size(1) <= self.pred_len and
                all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (data, tp, mask)) and
                tuple(mask.shape) == (B, L, C) and tuple(tp.shape) == (B, L) and timemixer_supported(*dims)):
            return False
        # the module itself: a .half() / .bfloat16() model, one left on another device, a non-contiguous parameter -> composed
        return all(q.device == data.device and q.dtype == torch.float32 and q.is_contiguous() for q in timemixer_params(self))

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        B, L, C = observed_data.shape
        assert C == self.C
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            if L < self.input_len and B > self.zeros_pad.shape[0]:      # the reference pads from batch_size rows of zeros: it fails here
                raise RuntimeError(f"TimeMixer: {B} windows of {L} < input_len {self.input_len} steps, but the padding buffer has "
                                   f"batch_size = {self.zeros_pad.shape[0]} rows")
            self.fused_calls += 1
            return timemixer_forecast(self, observed_data, observed_mask, observed_tp, tp_to_predict.size(1))
        if L < self.input_len:
            n = self.input_len - L
            observed_data = torch.cat([observed_data, self.zeros_pad[:B, :n, :]], dim=1)
            observed_mask = torch.cat([observed_mask, self.zeros_pad[:B, :n, :]], dim=1)
            observed_tp = torch.cat([observed_tp, self.zeros_pad[:B, :n, 0]], dim=1)
        Lp = tp_to_predict.size(1)      # the reference pads the horizon times to pred_len and never reads them
        x, means, stdev = masked_instance_norm(observed_data, observed_mask)
        enc_in = torch.cat([x, observed_mask, observed_tp.unsqueeze(-1)], dim=-1)
        enc = [self.enc_embedding(xi, None) for xi in self._multi_scale(enc_in)]
        for j, block in enumerate(self.pdm_blocks):
            enc = block(enc, last=j == self.layers - 1)
        head = self.predict_layers[-1]
        dec = linear(enc[-1].permute(0, 2, 1), head.weight, head.bias).permute(0, 2, 1)
        dec = linear(dec, self.projection.weight, self.projection.bias)
        dec = dec * stdev + means
        return dec[:, :Lp, :]


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
