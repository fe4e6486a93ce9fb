"""FullAttention / ProbAttention / AttentionLayer on MI355X (reference layers/SelfAttention_Family.py:50-77, 80-178, 181-215).

scores = einsum("blhe,bshe->bhls") and V = einsum("bhls,bshd->blhd") run as batched MFMA GEMMs over (batch, head)
directly on the (B,L,H,E) layout (no permutes/copies); softmax(scale*scores) + attention dropout is one fused row
kernel whose Philox mask is regenerated in backward.  `mask_flag=True` without an explicit mask is the causal
TriangularCausalMask (utils/masking.py); explicit attn_mask tensors are not on any configured path.  ProbAttention (Informer) is two launches per direction
(immtsf.ops.prob_attention, csrc/prob_attn.hip).
"""
from math import ceil, log, sqrt

import torch
import torch.nn as nn

from immtsf import config
from immtsf.ops import full_attention, linear, linear_multi, prob_attention


class FullAttention(nn.Module):
    _next_site = 0

    def __init__(self, mask_flag=True, factor=5, scale=None, attention_dropout=0.1, output_attention=False):
        super().__init__()
        self.scale = scale
        self.mask_flag = mask_flag
        self.output_attention = output_attention
        self.dropout = nn.Dropout(attention_dropout)
        self.p_drop = float(attention_dropout)
        self.site = 16 + (FullAttention._next_site % 1024)     # a Philox subsequence per attention instance
        FullAttention._next_site += 1
        self.precision = None

    def forward(self, queries, keys, values, attn_mask, tau=None, delta=None):
        if self.output_attention:
            raise NotImplementedError("output_attention=True is not provided by the fused path")
        if self.mask_flag and attn_mask is not None:
            raise NotImplementedError("explicit attn_mask tensors are not supported; mask_flag=True means causal")
        E = queries.shape[-1]
        scale = self.scale or 1.0 / sqrt(E)
        training = self.training and self.p_drop > 0.0
        seed = config.next_seed() if training else 0
        out = full_attention(queries, keys, values, scale, self.p_drop, training, seed, self.site, self.mask_flag,
                             self.precision)
        return out, None


class ProbAttention(nn.Module):
    """Informer's ProbSparse attention with the reference's constructor and forward signature.

    U_part = min(factor ceil(ln L_K), L_K) keys are sampled per query -- one (L_Q, U_part) sample for every batch and head -- the
    sparsity measure M = max - sum / L_K (the divisor is L_K; a key drawn twice counts twice) ranks the queries, the
    u = min(factor ceil(ln L_Q), L_Q) highest per (batch, head) get softmax(scale q K^T) V (mask_flag: key j > i masked for query i),
    every other row gets mean(V), or with mask_flag (L_Q == L_V asserted) the running sum of V.  `self.dropout` is never applied (as in
    the reference), and attn_mask is ignored: the reference builds its own ProbMask.  The result is (B, H, L_Q, D) contiguous:
    AttentionLayer reshapes it to (B, L, H D) WITHOUT a transpose, which is part of the reference's function (its state dicts were
    trained with it).

    Two definitions the reference leaves open:
      * ties in M: the lower query index wins, and the selected set is kept in ascending order (torch.topk(sorted=False) promises
        neither; the result does not depend on the order, only on the set);
      * the `.squeeze()` in `_prob_QK`: the un-squeezed meaning is implemented.  It differs from the reference only for n_heads == 1
        with B > 1, for U_part == 1 and for L_Q == 1, where the reference is wrong-shaped or fails.

    The sample: eagerly, torch.randint(L_K, (L_Q, U_part)) on the CPU default generator, once per call and in every case (u == L_Q
    included), so the same torch.manual_seed gives the reference's samples call for call; it is uploaded as int32.  While the current
    stream is capturing it is drawn on the device by torch's graph-safe generator (a replay draws a fresh one).  `sample_override`
    (an integer tensor (L_Q, U_part), or None; already on the device when a graph is captured) replaces the draw; `last_index_sample` keeps what was used, on the device."""

    def __init__(self, mask_flag=True, factor=5, scale=None, attention_dropout=0.1, output_attention=False):
        super().__init__()
        self.factor = factor
        self.scale = scale
        self.mask_flag = mask_flag
        self.output_attention = output_attention
        self.dropout = nn.Dropout(attention_dropout)
        self.sample_override = None
        self.last_index_sample = None

    def forward(self, queries, keys, values, attn_mask, tau=None, delta=None):
        if self.output_attention:
            raise NotImplementedError("output_attention=True is not provided by the fused path")
        B, L_Q, H, D = queries.shape
        L_K = keys.shape[1]
        U_part = min(self.factor * ceil(log(L_K)), L_K)
        u = min(self.factor * ceil(log(L_Q)), L_Q)
        if U_part < 1 or u < 1:
            raise ValueError(f"ProbAttention needs at least one sampled key and one selected query (L_Q {L_Q}, L_K {L_K}, factor {self.factor})")
        if self.mask_flag:
            assert L_Q == values.shape[1]
        if self.sample_override is not None:
            sample = self.sample_override
            if tuple(sample.shape) != (L_Q, U_part):
                raise ValueError(f"sample_override is {tuple(sample.shape)}, this call needs {(L_Q, U_part)}")
            sample = sample.to(device=queries.device, dtype=torch.int32)
        elif queries.is_cuda and torch.cuda.is_current_stream_capturing():
            sample = torch.randint(L_K, (L_Q, U_part), device=queries.device, dtype=torch.int32)
        else:
            sample = torch.randint(L_K, (L_Q, U_part)).to(device=queries.device, dtype=torch.int32)
        self.last_index_sample = sample
        scale = self.scale or 1.0 / sqrt(D)
        return prob_attention(queries, keys, values, sample, u, scale, self.mask_flag), None


class AttentionLayer(nn.Module):
    def __init__(self, attention, d_model, n_heads, d_keys=None, d_values=None):
        super().__init__()
        d_keys = d_keys or (d_model // n_heads)
        d_values = d_values or (d_model // n_heads)
        self.inner_attention = attention
        self.query_projection = nn.Linear(d_model, d_keys * n_heads)
        self.key_projection = nn.Linear(d_model, d_keys * n_heads)
        self.value_projection = nn.Linear(d_model, d_values * n_heads)
        self.out_projection = nn.Linear(d_values * n_heads, d_model)
        self.n_heads = n_heads

    def forward(self, queries, keys, values, attn_mask, tau=None, delta=None):
        B, L, _ = queries.shape
        S, H = keys.shape[1], self.n_heads
        prec = getattr(self.inner_attention, "precision", None)
        if queries is keys and keys is values:      # self-attention: the three projections share their input -- one launch (bf16 mode)
            q, k, v = linear_multi(queries, [self.query_projection.weight, self.key_projection.weight, self.value_projection.weight],
                                   [self.query_projection.bias, self.key_projection.bias, self.value_projection.bias], prec)
            q, k, v = q.view(B, L, H, -1), k.view(B, S, H, -1), v.view(B, S, H, -1)
        else:
            q = linear(queries, self.query_projection.weight, self.query_projection.bias, prec).view(B, L, H, -1)
            k = linear(keys, self.key_projection.weight, self.key_projection.bias, prec).view(B, S, H, -1)
            v = linear(values, self.value_projection.weight, self.value_projection.bias, prec).view(B, S, H, -1)
        out, attn = self.inner_attention(q, k, v, attn_mask, tau=tau, delta=delta)
        return linear(out.reshape(B, L, -1), self.out_projection.weight, self.out_projection.bias, prec), attn


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
