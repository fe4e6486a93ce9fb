#!/usr/bin/env python3
"""Generate tests/golden/model_dlinear_individual.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE): DLinear with
individual=True on the batch of make_golden.py's gen_models() -- B 3, L 6, Lp 4, C 3, input_len 8, pred_len 6, moving_avg 5 -- with the
weights perturbed from their constant init so that the channels (and the three maps) differ.

    python tests/golden/make_golden_dlinear.py

Like make_golden.py it imports the unmodified reference module at run time and stores tensors only (state_dict, inputs, output, upstream
gradient, parameter gradients): data, no code.
"""
import importlib
import types

import torch

import make_golden as G


def main():
    G._install_shims()
    g = torch.Generator().manual_seed(51)
    B, L, Lp, K = 3, 6, 4, 3
    data = torch.randn(B, L, K, generator=g)
    mask = (torch.rand(B, L, K, generator=g) < 0.7).float()
    data = data * mask
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
    cfg = types.SimpleNamespace(input_len=8, pred_len=6, enc_in=K, c_out=K, batch_size=4, device="cpu", moving_avg=5)
    torch.manual_seed(53)
    m = importlib.import_module("models.DLinear").DLinear(cfg, individual=True)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    m.train()
    out = m.forecasting(tpp, data.clone(), tp, mask)
    up = torch.randn(out.shape, generator=g)
    (out * up).sum().backward()
    arrs = dict(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), out=G._np(out), upstream=G._np(up))
    for k, v in m.state_dict().items():
        arrs[f"p.{k}"] = G._np(v)
    for k, p in m.named_parameters():
        arrs[f"g.{k}"] = G._np(p.grad)
    G.save("model_dlinear_individual", **arrs)


if __name__ == "__main__":
    main()
