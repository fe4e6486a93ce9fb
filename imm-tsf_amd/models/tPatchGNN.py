"""tPatchGNN backbone with the reference's constructor / forecasting signature and state_dict keys
(models/tPatchGNN.py:86-293), device-agnostic (the reference hard-codes .cuda() for the node vectors, :131-132).

On the hot path is the time-aware patch encoder: LearnableTE (:176-180) + TTCN
(:182-195), a masked softmax over each patch's irregular observations: the fused HIP kernel
(immtsf.ops.ttcn_patch_encode).  The per-patch transformer layer, the adaptive-graph stage and the forecast decoder run
on the HIP GEMM / LayerNorm / attention ops and the single-kernel graph-stage / decoder ops.  There is no eager or CPU
formulation in this module: the plain-torch restatement used to check it lives in oracle/tpatchgnn_ref.py (tests only).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from immtsf.dropin import fp32_entry as _fp32_entry


class nconv(nn.Module):
    def forward(self, x, A):            # x (B,F,N,M), A (B,M,N,V) -> (B,F,V,M)
        return torch.einsum("bfnm,bmnv->bfvm", x, A).contiguous()


class linear(nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.mlp = nn.Conv2d(c_in, c_out, kernel_size=(1, 1), padding=(0, 0), stride=(1, 1), bias=True)

    def forward(self, x):
        return self.mlp(x)


class gcn(nn.Module):
    def __init__(self, c_in, c_out, dropout, support_len=3, order=2):
        super().__init__()
        self.nconv = nconv()
        self.mlp = linear((order * support_len + 1) * c_in, c_out)
        self.dropout = dropout
        self.order = order

    def forward(self, x, support):
        feats = [x]
        for a in support:
            xk = x
            for _ in range(self.order):
                xk = self.nconv(xk, a)
                feats.append(xk)
        return F.relu(self.mlp(torch.cat(feats, dim=1)))


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, max_len=512):
        super().__init__()
        pe = torch.zeros(max_len, d_model)
        pos = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return x + self.pe[:, :x.size(1), :]


class tPatchGNN(nn.Module):
    immtsf_graphable = True      # no host syncs / data-dependent shapes in forecasting(): a step may be captured into a hipGraph

    def __init__(self, args, supports=None, dropout=0):
        super().__init__()
        self.device = args.device
        self.hid_dim = args.hid_dim
        self.N = args.C
        self.M = args.npatch
        self.batch_size = None
        self.supports = supports if supports is not None else []
        self.n_layer = args.nlayer
        self.te_dim = args.te_dim

        self.te_scale = nn.Linear(1, 1)
        self.te_periodic = nn.Linear(1, args.te_dim - 1)

        input_dim = 1 + args.te_dim
        ttcn_dim = args.hid_dim - 1
        self.ttcn_dim = ttcn_dim
        self.Filter_Generators = nn.Sequential(
            nn.Linear(input_dim, ttcn_dim, bias=True), nn.ReLU(inplace=True),
            nn.Linear(ttcn_dim, ttcn_dim, bias=True), nn.ReLU(inplace=True),
            nn.Linear(ttcn_dim, input_dim * ttcn_dim, bias=True))
        self.T_bias = nn.Parameter(torch.randn(1, ttcn_dim))

        d_model = args.hid_dim
        self.ADD_PE = PositionalEncoding(d_model)
        self.transformer_encoder = nn.ModuleList()
        for _ in range(self.n_layer):
            layer = nn.TransformerEncoderLayer(d_model=d_model, nhead=args.n_heads, batch_first=True)
            self.transformer_encoder.append(nn.TransformerEncoder(layer, num_layers=args.tf_layer))

        self.supports_len = len(self.supports) + 1
        self.nodevec_dim = args.node_dim
        self.nodevec1 = nn.Parameter(torch.randn(self.N, args.node_dim), requires_grad=True)
        self.nodevec2 = nn.Parameter(torch.randn(args.node_dim, self.N), requires_grad=True)
        self.nodevec_linear1 = nn.ModuleList()
        self.nodevec_linear2 = nn.ModuleList()
        self.nodevec_gate1 = nn.ModuleList()
        self.nodevec_gate2 = nn.ModuleList()
        for _ in range(self.n_layer):
            self.nodevec_linear1.append(nn.Linear(args.hid_dim, args.node_dim))
            self.nodevec_linear2.append(nn.Linear(args.hid_dim, args.node_dim))
            self.nodevec_gate1.append(nn.Sequential(nn.Linear(args.hid_dim + args.node_dim, 1), nn.Tanh(), nn.ReLU()))
            self.nodevec_gate2.append(nn.Sequential(nn.Linear(args.hid_dim + args.node_dim, 1), nn.Tanh(), nn.ReLU()))
        self.gconv = nn.ModuleList(
            [gcn(d_model, d_model, dropout, support_len=self.supports_len, order=args.hop) for _ in range(self.n_layer)])

        self.outlayer = args.outlayer
        enc_dim = args.hid_dim
        if self.outlayer == "Linear":
            self.temporal_agg = nn.Sequential(nn.Linear(args.hid_dim * self.M, enc_dim))
        elif self.outlayer == "CNN":
            self.temporal_agg = nn.Sequential(nn.Conv1d(d_model, enc_dim, kernel_size=self.M))
        self.decoder = nn.Sequential(
            nn.Linear(enc_dim + args.te_dim, args.hid_dim), nn.ReLU(inplace=True),
            nn.Linear(args.hid_dim, args.hid_dim), nn.ReLU(inplace=True),
            nn.Linear(args.hid_dim, 1))

    # ---- time-aware patch encoder ---------------------------------------------------------------
    def LearnableTE(self, tt):
        """[w0 t + b0 ; sin(W t + b)] (reference :176-180): one HIP kernel forward, two backward"""
        from immtsf.ops import time2vec
        return time2vec(tt.squeeze(-1), self.te_scale.weight, self.te_scale.bias, self.te_periodic.weight, self.te_periodic.bias)

    def _encode_patches(self, x, tt, mask):
        """x, tt, mask: (P, L) -> (P, hid_dim) patch embedding incl. the patch-non-empty flag: the fused TE + TTCN kernel
        (raises on CPU tensors: there is no fallback)"""
        from immtsf.ops import ttcn_patch_encode
        lin = self.Filter_Generators
        return ttcn_patch_encode(x, tt, mask, self.te_scale.weight, self.te_scale.bias, self.te_periodic.weight,
                                 self.te_periodic.bias, lin[0].weight, lin[0].bias, lin[2].weight, lin[2].bias,
                                 lin[4].weight, lin[4].bias, self.T_bias, with_flag=True)     # flag column written in-kernel

    # ---- transformer + adaptive-graph GCN over (variables x patches) ------------------------------
    def _encoder_layer_hip(self, lyr, x):
        """one post-norm nn.TransformerEncoderLayer (relu FFN, batch_first) evaluated from ITS parameters on the HIP
        GEMM / LayerNorm / attention kernels: at d_model=32 with dim_feedforward=2048 the stock path spends its time
        in badly-shaped library GEMMs.  Dropout uses torch's generator exactly like the stock layer."""
        from immtsf.ops import full_attention_qkv, layer_norm, linear
        Bs, S, D = x.shape
        at = lyr.self_attn
        H = at.num_heads
        qkv = linear(x, at.in_proj_weight, at.in_proj_bias).view(Bs, S, 3, H, D // H)
        p_att = at.dropout if self.training else 0.0
        from immtsf import config
        a = full_attention_qkv(qkv, 1.0 / math.sqrt(D // H), p_att, self.training,
                               config.next_seed() if p_att > 0 else 0, 900)
        sa = linear(a.reshape(Bs, S, D), at.out_proj.weight, at.out_proj.bias)
        x = layer_norm(x + lyr.dropout1(sa), lyr.norm1.weight, lyr.norm1.bias, lyr.norm1.eps)
        ff = linear(lyr.dropout(linear(x, lyr.linear1.weight, lyr.linear1.bias, relu=True)), lyr.linear2.weight, lyr.linear2.bias)
        return layer_norm(x + lyr.dropout2(ff), lyr.norm2.weight, lyr.norm2.bias, lyr.norm2.eps)

    def _transformer(self, layer, x):
        from immtsf.ops import SITE_LAYER_BASE, encoder_layer, encoder_layer_supported
        enc = self.transformer_encoder[layer]
        for li, lyr in enumerate(enc.layers):
            if encoder_layer_supported(x.shape[1], x.shape[2], lyr.self_attn.num_heads):
                # the whole layer behind one entry point per direction (csrc/encoder_layer.hip): 7 + 15 launches instead of 13 + ~24
                x = encoder_layer(lyr, x, self.training, SITE_LAYER_BASE + 64 + 8 * (layer * len(enc.layers) + li))
            else:
                x = self._encoder_layer_hip(lyr, x)
        return x if enc.norm is None else enc.norm(x)

    def _mlp(self, seq, x):
        """nn.Sequential of Linear/ReLU evaluated on the HIP GEMM"""
        from immtsf.ops import linear, mlp
        mods = list(seq)
        if all(isinstance(m, nn.Linear if i % 2 == 0 else nn.ReLU) for i, m in enumerate(mods)) and len(mods) % 2 == 1:
            lins = mods[0::2]
            return mlp(x, [m.weight for m in lins], [m.bias for m in lins])
        for m in mods:
            x = linear(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
        return x

    def _graph_stage(self, layer, x):
        """node-vector gating -> adaptive adjacency -> graph convolution -> 1x1 mixing (reference :212-236), (B,N,M,D).
        One fused kernel per direction when a (window, patch) cell's operands fit a CU's LDS (every BASELINE configuration);
        larger variable counts, or externally supplied `supports`, take the stock-torch formulation below -- the module's tested
        behaviour for such shapes (tests/test_gpu_backbone.py::test_out_of_limit_shapes_take_the_tested_unfused_paths), not a
        silent substitute for a missing extension: the fused path raises when the library is absent."""
        B, N, M, D = x.shape
        gc = self.gconv[layer]
        if not self.supports:
            from immtsf.ops import gcn_adaptive, gcn_adaptive_supported
            if gcn_adaptive_supported(N, D, self.nodevec_dim, gc.order):     # one cell's operands fit a CU's LDS
                return gcn_adaptive(x, gc.order, self.nodevec1, self.nodevec2, self.nodevec_gate1[layer][0],
                                    self.nodevec_gate2[layer][0], self.nodevec_linear1[layer],
                                    self.nodevec_linear2[layer], gc.mlp.mlp)
        nv1 = self.nodevec1.view(1, 1, N, self.nodevec_dim).expand(B, M, N, self.nodevec_dim)
        nv2 = self.nodevec2.view(1, 1, self.nodevec_dim, N).expand(B, M, self.nodevec_dim, N)
        g1 = self.nodevec_gate1[layer](torch.cat([x, nv1.permute(0, 2, 1, 3)], dim=-1))
        g2 = self.nodevec_gate2[layer](torch.cat([x, nv2.permute(0, 3, 1, 2)], dim=-1))
        p1 = g1 * self.nodevec_linear1[layer](x)
        p2 = g2 * self.nodevec_linear2[layer](x)
        nv1 = nv1 + p1.permute(0, 2, 1, 3)
        nv2 = nv2 + p2.permute(0, 2, 3, 1)
        adp = F.softmax(F.relu(torch.matmul(nv1, nv2)), dim=-1)
        return gc(x.permute(0, 3, 1, 2), self.supports + [adp]).permute(0, 2, 3, 1)

    def IMTS_Model(self, x_patch):
        B, N, M, D = x_patch.shape
        x = x_patch
        for layer in range(self.n_layer):
            x_last = x if layer > 0 else None
            x = self._transformer(layer, self.ADD_PE(x.reshape(B * N, M, D))).view(B, N, M, D)
            x = self._graph_stage(layer, x)
            if x_last is not None:
                x = x_last + x
        if self.outlayer == "CNN":
            x = self.temporal_agg(x.reshape(B * N, M, -1).permute(0, 2, 1)).view(B, N, -1)
        else:
            x = self._mlp(self.temporal_agg, x.reshape(B, N, -1))
        return x

    @_fp32_entry
    def forecasting(self, time_steps_to_predict, X, truth_time_steps, mask=None):
        """time_steps_to_predict (B,Lp); X, truth_time_steps, mask (B,M,L,N) -> (B,Lp,N)"""
        B, M, L, N = X.shape
        self.batch_size = B
        if X.is_cuda and not (X.requires_grad or truth_time_steps.requires_grad) and mask is not None and mask.shape == X.shape \
                and truth_time_steps.shape == X.shape:
            from immtsf.ops import patch_flatten3
            fx, ft, fm = patch_flatten3(X, truth_time_steps, mask)          # one launch for the three (B,M,L,N) -> (B*N*M, L) copies
        else:
            flat = lambda t: t.permute(0, 3, 1, 2).reshape(B * N * M, L)    # noqa: E731
            fx, ft, fm = flat(X), flat(truth_time_steps), flat(mask)
        x_patch = self._encode_patches(fx, ft, fm).view(B, N, M, -1)
        h = self.IMTS_Model(x_patch)                                     # (B,N,hid)
        Lp = time_steps_to_predict.shape[-1]
        # the reference repeats the prediction times over the N variables before embedding them (:283-285); the
        # embedding is the same for every variable, so embed once per window
        from immtsf.ops import tpatch_decoder, tpatch_decoder_supported, tpatch_decoder_te
        fits = tpatch_decoder_supported(self.decoder, N, Lp, h.shape[-1], self.te_dim)
        if fits and self.te_dim <= 16 and not time_steps_to_predict.requires_grad:
            # (B,Lp,N), one kernel: LearnableTE of the prediction times is computed inside, its gradients come out of the backward kernel
            return tpatch_decoder_te(self.decoder, h, time_steps_to_predict.reshape(B, Lp), self.te_scale.weight, self.te_scale.bias,
                                     self.te_periodic.weight, self.te_periodic.bias)
        te = self.LearnableTE(time_steps_to_predict.view(B, 1, Lp, 1))                     # (B,1,Lp,te_dim)
        if fits:
            return tpatch_decoder(self.decoder, h, te.view(B, Lp, self.te_dim))          # (B,Lp,N), one kernel
        te_pred = te.expand(B, N, Lp, self.te_dim)                                         # expand's backward sums over N
        h = torch.cat([h.unsqueeze(2).expand(B, N, Lp, h.shape[-1]), te_pred], dim=-1)
        return self._mlp(self.decoder, h).squeeze(-1).permute(0, 2, 1)


from immtsf.dropin import reexport_missing as _reexport_missing  # noqa: E402

_reexport_missing(globals())     # names of the reference module this build does not mirror
