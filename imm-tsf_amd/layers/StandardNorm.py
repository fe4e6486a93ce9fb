"""Reversible instance normalisation (reference layers/StandardNorm.py:5-68): `norm` takes the statistics over every axis but the first
and the last and normalises with them, `denorm` undoes it with the statistics of the last `norm` call.  Same constructor, same
parameter names (`affine_weight`, `affine_bias`).  TimeMixer constructs one per scale and never calls them; plain torch."""
import torch
import torch.nn as nn


class Normalize(nn.Module):
    def __init__(self, num_features: int, eps=1e-5, affine=False, subtract_last=False, non_norm=False):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.affine = affine
        self.subtract_last = subtract_last
        self.non_norm = non_norm
        if affine:
            self.affine_weight = nn.Parameter(torch.ones(num_features))
            self.affine_bias = nn.Parameter(torch.zeros(num_features))

    def forward(self, x, mode: str):
        if mode == "norm":
            dims = tuple(range(1, x.ndim - 1))
            if self.subtract_last:
                self.last = x[:, -1, :].unsqueeze(1)
            else:
                self.mean = torch.mean(x, dim=dims, keepdim=True).detach()
            self.stdev = torch.sqrt(torch.var(x, dim=dims, keepdim=True, unbiased=False) + self.eps).detach()
            if self.non_norm:
                return x
            x = (x - (self.last if self.subtract_last else self.mean)) / self.stdev
            return x * self.affine_weight + self.affine_bias if self.affine else x
        if mode == "denorm":
            if self.non_norm:
                return x
            if self.affine:
                x = (x - self.affine_bias) / (self.affine_weight + self.eps * self.eps)
            return x * self.stdev + (self.last if self.subtract_last else self.mean)
        raise NotImplementedError


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
