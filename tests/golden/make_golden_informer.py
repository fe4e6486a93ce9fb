#!/usr/bin/env python3
"""Generate tests/golden/model_informer.npz, model_informer_nodistil.npz and layer_conv_distil.npz from the REAL reference (its checkout at
$IMMTSF_REFERENCE): models.Informer.Informer in train mode at dropout 0, with every parameter perturbed from its init by 0.1 randn, and
layers.Transformer_EncDec.ConvLayer alone.

    python tests/golden/make_golden_informer.py

    fixture                  B  L   Lp  C  input_len  pred_len  d_model  heads  d_ff  e/d layers  factor  distil  activation
    model_informer           3  10  4   3  12         5         16       2      32    2/1         1       yes     gelu    both paddings taken;
                                                                                    u = 3 < 12 in the encoder; the cross-attention sees 7 keys
    model_informer_nodistil  3  12  4   3  12         5         16       4      32    3/1         3       no      relu    L == input_len; every
                                                                                    query is selected in the decoder
    layer_conv_distil        ConvLayer at (B, L, d) = (1, 2, 4) and (3, 9, 8): evaluation and training forward + backward, buffers before/after

Like make_golden.py it imports the unmodified reference modules at run time and stores tensors only: data, no code.  Every torch.randint
draw of ProbAttention is recorded by wrapping torch.randint here (`sample.<call>`, in call order), and per call the smallest gap, over
(batch, head), between the u-th and (u+1)-th largest sparsity measure relative to max|M| (`gap`, inf where every query is selected).  A
seed whose smallest gap is below 1e-3 is refused -- fp32 cannot then flip the selection -- and the next one is tried.
"""
import copy
import importlib
import types

import numpy as np
import torch

import make_golden as G

MIN_GAP = 1e-3
COMMON = dict(C=3, c_out=3, input_len=12, pred_len=5, d_model=16, d_ff=32, d_layers=1, embed="fixed", freq="h")
FIXTURES = {      # name: (B, L, Lp, first seed, options)
    "model_informer": (3, 10, 4, 83, dict(COMMON, n_heads=2, e_layers=2, factor=1, distil=True, activation="gelu")),
    "model_informer_nodistil": (3, 12, 4, 89, dict(COMMON, n_heads=4, e_layers=3, factor=3, distil=False, activation="relu")),
}
CONV_CASES = {"a": (1, 2, 4, 97), "b": (3, 9, 8, 101)}      # name: (B, L, d, seed)


def config(batch_size=4, device="cpu", dropout=0.0, **opts):
    return types.SimpleNamespace(batch_size=batch_size, device=device, dropout=dropout, **opts)


def run_model(Informer, SAF, B, L, Lp, seed, opts):
    C = opts["C"]
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    data = data * mask
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
    torch.manual_seed(seed + 2)
    m = Informer(config(**opts))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    m.train()
    before = copy.deepcopy(m.state_dict())
    samples, gaps = [], []
    real_randint, real_prob = torch.randint, SAF.ProbAttention._prob_QK

    def randint(*a, **k):
        r = real_randint(*a, **k)
        samples.append(r.clone())
        return r

    def prob_qk(self, Q, K, sample_k, n_top):
        r = real_prob(self, Q, K, sample_k, n_top)
        s = samples[-1]
        LQ, LK = Q.shape[2], K.shape[2]
        QK = torch.einsum("bhld,bhlud->bhlu", Q.detach().double(), K.detach().double()[:, :, s, :])
        M = QK.max(-1).values - QK.sum(-1) / LK
        if n_top < LQ:
            top = torch.sort(M, -1, descending=True).values
            gaps.append(float(((top[..., n_top - 1] - top[..., n_top]) / M.abs().amax(-1)).min()))
        else:
            gaps.append(float("inf"))
        return r

    torch.randint, SAF.ProbAttention._prob_QK = randint, prob_qk
    try:
        torch.manual_seed(seed)
        out = m.forecasting(tpp, data.clone(), tp, mask)
    finally:
        torch.randint, SAF.ProbAttention._prob_QK = real_randint, real_prob
    up = torch.randn(out.shape, generator=g)
    (out * up).sum().backward()
    arrs = dict(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), out=G._np(out), upstream=G._np(up), seed=np.array(seed),
                gap=np.array(gaps))
    for i, s in enumerate(samples):
        arrs[f"sample.{i}"] = s.numpy().astype(np.int32)
    for key, v in before.items():
        arrs[f"p.{key}"] = G._np(v)
    for key, v in m.state_dict().items():
        if "running_" in key or "num_batches" in key:
            arrs[f"after.{key}"] = G._np(v)
    none = []
    for key, p in m.named_parameters():
        if p.grad is None:
            none.append(key)
        else:
            arrs[f"g.{key}"] = G._np(p.grad)
    arrs["none"] = np.array("\n".join(none))
    return min(gaps), arrs


def run_conv(ConvLayer, B, L, d, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed + 2)
    m = ConvLayer(d)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        m.norm.running_mean.copy_(0.1 * torch.randn(d, generator=g))
        m.norm.running_var.copy_(1 + 0.2 * torch.rand(d, generator=g))
    x = torch.randn(B, L, d, generator=g)
    arrs = {"x": G._np(x)}
    for key, v in m.state_dict().items():
        arrs[f"p.{key}"] = G._np(v).copy()      # (the training call below updates the buffers in place)
    for mode in ("eval", "train"):
        m.train(mode == "train")
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        out = m(xi)
        up = torch.randn(out.shape, generator=g)
        (out * up).sum().backward()
        arrs.update({f"{mode}.out": G._np(out), f"{mode}.upstream": G._np(up), f"{mode}.gx": G._np(xi.grad)})
        for key, p in m.named_parameters():
            arrs[f"{mode}.g.{key}"] = G._np(p.grad)
    for key, v in m.state_dict().items():
        if "running_" in key or "num_batches" in key:
            arrs[f"after.{key}"] = G._np(v)
    return arrs


def main():
    G._install_shims()
    SAF = importlib.import_module("layers.SelfAttention_Family")
    Informer = importlib.import_module("models.Informer").Informer
    ConvLayer = importlib.import_module("layers.Transformer_EncDec").ConvLayer
    for name, (B, L, Lp, seed, opts) in FIXTURES.items():
        for s in range(seed, seed + 50):
            gap, arrs = run_model(Informer, SAF, B, L, Lp, s, opts)
            if gap >= MIN_GAP:
                break
            print(f"{name}: seed {s} refused (smallest gap {gap:.2e})")
        else:
            raise SystemExit(f"{name}: no seed with a gap of {MIN_GAP}")
        print(f"{name}: seed {s}, gaps {arrs['gap']}")
        G.save(name, **arrs)
    conv = {}
    for case, (B, L, d, seed) in CONV_CASES.items():
        for k, v in run_conv(ConvLayer, B, L, d, seed).items():
            conv[f"{case}.{k}"] = v
    G.save("layer_conv_distil", **conv)


if __name__ == "__main__":
    main()
