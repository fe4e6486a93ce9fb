"""DLinear backbone (reference models/DLinear.py:7-134): masked instance norm, moving-average decomposition, three
Linear(seq_len -> pred_len) maps on (seasonal, trend, timestamps).  Same signature/state_dict.

forecasting() is ONE HIP launch (immtsf.ops.dlinear_forecast, csrc/dlinear.hip: the padding to input_len, the normalisation, the
decomposition, the three maps, the de-normalisation and the slice to the horizon) and its backward TWO (parameter gradients only, summed
in a fixed order) whenever config.dlinear_fused is on, the tensors are fp32 on the GPU, immtsf_dlinear_supported takes the shapes
(input_len, pred_len <= 128, odd moving_avg) and neither data, mask nor times wants a gradient; `fused_calls` counts those calls.
Anything else -- and IMMTSF_DLINEAR_FUSED=0 -- runs the composed path: torch element-wise ops around three immtsf.ops.linear calls (one
HIP GEMM each; C of them per map in individual mode).  The fused path is fp32 in bf16 mode too."""
import torch
import torch.nn as nn

from immtsf import config
from immtsf.ops import dlinear_forecast, dlinear_supported, linear
from immtsf.dropin import fp32_entry as _fp32_entry
from layers.Autoformer_EncDec import series_decomp
from models._common import masked_instance_norm


class DLinear(nn.Module):
    immtsf_graphable = True      # no host syncs / data-dependent shapes in forecasting()

    def __init__(self, configs, individual=False):
        super().__init__()
        self.input_len = configs.input_len
        self.seq_len = configs.input_len
        self.pred_len = configs.pred_len
        self.individual = individual
        self.C = configs.enc_in
        self.decomposition = series_decomp(configs.moving_avg)

        def make():
            lin = nn.Linear(self.seq_len, self.pred_len)
            lin.weight = nn.Parameter((1 / self.seq_len) * torch.ones_like(lin.weight))
            return lin
        if individual:
            self.Linear_Seasonal = nn.ModuleList([make() for _ in range(self.C)])
            self.Linear_Trend = nn.ModuleList([make() for _ in range(self.C)])
            self.Linear_Time = nn.ModuleList([make() for _ in range(self.C)])
        else:
            self.Linear_Seasonal, self.Linear_Trend, self.Linear_Time = make(), make(), make()
        self.zeros_pad = torch.zeros(configs.batch_size, max(self.seq_len, self.pred_len), self.C, device=configs.device)
        self.moving_avg = int(configs.moving_avg)
        self.fused_calls = 0         # forecasting() calls that took the fused HIP path (tests assert which path ran)

    def _project(self, lin, x):                                  # x (B, C, L) -> (B, C, pred_len)
        if self.individual:
            return torch.stack([linear(x[:, i, :], lin[i].weight, lin[i].bias) for i in range(self.C)], dim=1)
        return linear(x, lin.weight, lin.bias)

    def _fused_ok(self, tp_to_predict, data, tp, mask):
        B, L, C = data.shape
        return (config.dlinear_fused and B > 0 and L <= self.input_len and tp_to_predict.size(1) <= self.pred_len and
                all(t.is_cuda and t.dtype == torch.float32 and not t.requires_grad for t in (data, tp, mask)) and
                tuple(mask.shape) == (B, L, C) and tuple(tp.shape) == (B, L) and
                dlinear_supported(self.seq_len, self.pred_len, C, self.moving_avg, self.individual))

    @_fp32_entry
    def forecasting(self, tp_to_predict, observed_data, observed_tp, observed_mask):
        B, L, C = observed_data.shape
        assert C == self.C
        if self._fused_ok(tp_to_predict, observed_data, observed_tp, observed_mask):
            if L < self.input_len and B > self.zeros_pad.shape[0]:      # the reference pads from batch_size rows of zeros: it fails here
                raise RuntimeError(f"DLinear: {B} windows of {L} < input_len {self.input_len} steps, but the padding buffer has "
                                   f"batch_size = {self.zeros_pad.shape[0]} rows")
            self.fused_calls += 1
            return dlinear_forecast(observed_data, observed_mask, observed_tp, tp_to_predict.size(1), self.seq_len, self.pred_len,
                                    self.moving_avg, self.Linear_Seasonal, self.Linear_Trend, self.Linear_Time)
        if L < self.input_len:
            n = self.input_len - L
            observed_data = torch.cat([observed_data, self.zeros_pad[:B, :n, :]], dim=1)
            observed_mask = torch.cat([observed_mask, self.zeros_pad[:B, :n, :]], dim=1)
            observed_tp = torch.cat([observed_tp, self.zeros_pad[:B, :n, 0]], dim=1)
        Lp = tp_to_predict.size(1)
        x, means, stdev = masked_instance_norm(observed_data, observed_mask)
        seasonal, trend = self.decomposition(x)
        time = observed_tp.unsqueeze(1).expand(-1, C, -1)
        dec = (self._project(self.Linear_Seasonal, seasonal.permute(0, 2, 1)) +
               self._project(self.Linear_Trend, trend.permute(0, 2, 1)) +
               self._project(self.Linear_Time, time)).permute(0, 2, 1)
        dec = dec * stdev + means
        return dec[:, :Lp, :]


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
