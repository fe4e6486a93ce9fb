"""TTM's mixer layers (reference layers/MLP.py:4-121): same class names, constructors and state_dict keys.

A TTMMixerBlock normalises over the last axis, runs Linear(F -> 2F), exact GELU, dropout, Linear(2F -> F), dropout and a softmax gate
along ONE axis of x (B, M, N, D) -- patches (N), channels (M) or features (D) -- and adds the input back.  Block by block, whenever
config.ttm_fused is on, x and the block's parameters are contiguous fp32 tensors on one GPU and the limits allow:
  patch / channel   ONE HIP launch (immtsf.ops.ttm_mixer, csrc/ttm.hip; backward two), no permuted copy, dropout drawn in the kernel;
  feature           immtsf.ops.layer_norm, three immtsf.ops.linear GEMMs with torch's GELU / dropout between them, and ONE launch
                    for gate + residual (immtsf.ops.ttm_gate).
Anything else -- and IMMTSF_TTM_FUSED=0 -- runs the composed path: the reference's sequence with immtsf.ops.linear for every nn.Linear
and immtsf.ops.layer_norm for the norm.  `took_kernel` says which path a block's latest call ran.  The kernels are fp32 in bf16 mode too;
there only the GEMMs change, through linear()."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from immtsf import config
from immtsf.ops import layer_norm, linear, ttm_gate, ttm_mixer, ttm_mixer_params, ttm_mixer_supported


def _lin(layer, x):
    """nn.Linear on the HIP GEMM; a .half() / .bfloat16() layer's parameters are widened (the composed path computes in fp32)"""
    W, b = layer.weight, layer.bias
    if W.dtype != torch.float32:
        W, b = W.float(), None if b is None else b.float()
    return linear(x, W, b)


class TTMGatedLayer(nn.Module):
    def __init__(self, in_size, out_size):
        super().__init__()
        self.attn_layer = nn.Linear(in_size, out_size)
        self.attn_softmax = nn.Softmax(dim=-1)

    def forward(self, inputs):
        return inputs * self.attn_softmax(_lin(self.attn_layer, inputs))


class TTMMLP(nn.Module):
    def __init__(self, in_features, out_features, factor, dropout):
        super().__init__()
        self.fc1 = nn.Linear(in_features, in_features * factor)
        self.dropout1 = nn.Dropout(dropout)
        self.fc2 = nn.Linear(in_features * factor, out_features)
        self.dropout2 = nn.Dropout(dropout)

    def forward(self, inputs):
        inputs = self.dropout1(F.gelu(_lin(self.fc1, inputs)))
        return self.dropout2(_lin(self.fc2, inputs))


class TTMMixerBlock(nn.Module):
    def __init__(self, d_model, features, mode, dropout):
        super().__init__()
        self.mode = mode
        self.norm = nn.LayerNorm(d_model)
        self.mlp = TTMMLP(in_features=features, out_features=features, factor=2, dropout=dropout)
        self.gating_block = TTMGatedLayer(in_size=features, out_size=features)
        self.took_kernel = False     # the latest call ran csrc/ttm.hip (tests and TTM.fused_blocks read it)
        self._last_drop = None       # (p, seed, site, counter pointer) of the latest narrow-kernel call's dropout

    def _norm(self, x):
        if x.is_cuda and x.dtype == torch.float32 and x.numel() // x.shape[-1] < 2 ** 31:
            return layer_norm(x, self.norm.weight.float(), self.norm.bias.float(), self.norm.eps)
        return self.norm(x)

    def kernel_ok(self, x):
        """this call can take the HIP kernel of its mode"""
        if not (config.ttm_fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.numel() > 0):
            return False
        if any(q.device != x.device or q.dtype != torch.float32 or not q.is_contiguous() for q in ttm_mixer_params(self)):
            return False      # a .half() / .bfloat16() block, one on another device, a non-contiguous parameter
        if self.mode == "feature":
            return True
        return self.mlp.dropout1.p == self.mlp.dropout2.p and ttm_mixer_supported(self.mode, tuple(x.shape))

    def forward(self, x):
        assert self.mode in ["patch", "feature", "channel"]
        self.took_kernel = self.kernel_ok(x)
        if self.took_kernel and self.mode != "feature":
            return ttm_mixer(self, x, self.mode, self.training)
        if self.took_kernel:
            u = self.mlp(self._norm(x))
            return ttm_gate(x, u, _lin(self.gating_block.attn_layer, u))
        residual = x
        x = self._norm(x)
        if self.mode == "patch":
            x = x.permute(0, 1, 3, 2)
        elif self.mode == "channel":
            x = x.permute(0, 3, 2, 1)
        x = self.gating_block(self.mlp(x))
        if self.mode == "patch":
            x = x.permute(0, 1, 3, 2)
        elif self.mode == "channel":
            x = x.permute(0, 3, 2, 1)
        return x + residual


class TTMLayer(nn.Module):
    def __init__(self, d_model, num_patches, n_vars, mode, dropout):
        super().__init__()
        if num_patches > 1:      # one patch: nothing to mix, and no parameters for it
            self.patch_mixer = TTMMixerBlock(d_model=d_model, features=num_patches, mode="patch", dropout=dropout)
        self.feature_mixer = TTMMixerBlock(d_model=d_model, features=d_model, mode="feature", dropout=dropout)
        self.mode = mode
        self.num_patches = num_patches
        if self.mode == "mix_channel":
            self.channel_feature_mixer = TTMMixerBlock(d_model=d_model, features=n_vars, mode="channel", dropout=dropout)

    def forward(self, x):
        if self.mode == "mix_channel":
            x = self.channel_feature_mixer(x)
        if self.num_patches > 1:
            x = self.patch_mixer(x)
        return self.feature_mixer(x)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror (AutoTimesMLP)
