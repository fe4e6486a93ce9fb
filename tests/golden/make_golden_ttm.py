#!/usr/bin/env python3
"""Generate tests/golden/model_ttm.npz, model_ttm_odd.npz and model_ttm_plain.npz from the REAL reference (its checkout at
$IMMTSF_REFERENCE): models.TTM.TTM in train mode at dropout 0, with every parameter perturbed from its init by 0.1 randn.

    python tests/golden/make_golden_ttm.py

    fixture          B  L   Lp  C  input_len  pred_len  patch  stride  patches  d_model  AP  e/d layers  d_d_model  options
    model_ttm        3  6   4   3  8          6         2      2       4        16       2   2/2         8          mix_channel, decoder, norm
    model_ttm_odd    3  31  5   2  33         7         6      24      2        24       3   1/1         10         same; a dropped tail
    model_ttm_plain  3  6   4   3  8          6         2      8       1        16       0   2/-         -          common_channel, no decoder,
                                                                                                                    use_norm 0, no patch mixer

Like make_golden.py it imports the unmodified reference module at run time and stores tensors only (state_dict, inputs, output, upstream
gradient, parameter gradients, and -- as `none`, one name per line -- the parameters whose gradient is None): data, no code.
"""
import importlib
import types

import numpy as np
import torch

import make_golden as G

FIXTURES = {      # name: (B, L, Lp, seed, options)
    "model_ttm": (3, 6, 4, 71, dict(enc_in=3, input_len=8, pred_len=6, patch_size=2, stride=2, d_model=16, AP_levels=2, e_layers=2, d_layers=2,
                                    d_d_model=8, mode="mix_channel", use_decoder=True, use_norm=1)),
    "model_ttm_odd": (3, 31, 5, 73, dict(enc_in=2, input_len=33, pred_len=7, patch_size=6, stride=24, d_model=24, AP_levels=3, e_layers=1,
                                         d_layers=1, d_d_model=10, mode="mix_channel", use_decoder=True, use_norm=1)),
    "model_ttm_plain": (3, 6, 4, 79, dict(enc_in=3, input_len=8, pred_len=6, patch_size=2, stride=8, d_model=16, AP_levels=0, e_layers=2,
                                          d_layers=2, d_d_model=8, mode="common_channel", use_decoder=False, use_norm=0)),
}


def config(batch_size=4, device="cpu", dropout=0.0, **opts):
    return types.SimpleNamespace(batch_size=batch_size, device=device, dropout=dropout, **opts)


def main():
    G._install_shims()
    TTM = importlib.import_module("models.TTM").TTM
    for name, (B, L, Lp, seed, opts) in FIXTURES.items():
        C = opts["enc_in"]
        g = torch.Generator().manual_seed(seed)
        data = torch.randn(B, L, C, generator=g)
        mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
        data = data * mask
        tp = torch.sort(torch.rand(B, L, generator=g), 1).values
        tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
        torch.manual_seed(seed + 2)
        m = TTM(config(**opts))
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        m.train()
        out = m.forecasting(tpp, data.clone(), tp, mask)
        up = torch.randn(out.shape, generator=g)
        (out * up).sum().backward()
        arrs = dict(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), out=G._np(out), upstream=G._np(up))
        for key, v in m.state_dict().items():
            arrs[f"p.{key}"] = G._np(v)
        none = []
        for key, p in m.named_parameters():
            if p.grad is None:
                none.append(key)
            else:
                arrs[f"g.{key}"] = G._np(p.grad)
        arrs["none"] = np.array("\n".join(none))
        G.save(name, **arrs)


if __name__ == "__main__":
    main()
