#!/usr/bin/env python3
"""Generate tests/golden/model_timemixer.npz and model_timemixer_odd.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE):
TimeMixer at the reference's default options (moving_avg decomposition, channel independence, average pooling, window 2,
down_sampling_layers 3, embed timeF / freq h), train mode at dropout 0, with every parameter perturbed from its init so that no two
maps coincide.

    python tests/golden/make_golden_timemixer.py

    fixture                B  L   Lp  C  input_len  pred_len  d_model  d_ff  e_layers  moving_avg
    model_timemixer        3  6   4   3  8          6         8        12    2         5            scales 8, 4, 2, 1
    model_timemixer_odd    3  33  7   3  33         7         16       32    2         25           scales 33, 16, 8, 4: dropped tails

Like make_golden.py it imports the unmodified reference module at run time and stores tensors only (state_dict, inputs, output, upstream
gradient, parameter gradients, and -- as `none`, one name per line -- the parameters whose gradient is None): data, no code.
"""
import importlib
import types

import numpy as np
import torch

import make_golden as G

FIXTURES = {      # name: (B, L, Lp, C, input_len, pred_len, d_model, d_ff, e_layers, moving_avg, seed)
    "model_timemixer": (3, 6, 4, 3, 8, 6, 8, 12, 2, 5, 61),
    "model_timemixer_odd": (3, 33, 7, 3, 33, 7, 16, 32, 2, 25, 67),
}


def config(C, input_len, pred_len, d_model, d_ff, e_layers, moving_avg, batch_size=4, device="cpu", dropout=0.0, **over):
    cfg = types.SimpleNamespace(input_len=input_len, pred_len=pred_len, enc_in=C, c_out=C, batch_size=batch_size, device=device,
                                d_model=d_model, d_ff=d_ff, e_layers=e_layers, moving_avg=moving_avg, dropout=dropout, embed="timeF",
                                freq="h", top_k=5, decomp_method="moving_avg", channel_independence=1, down_sampling_layers=3,
                                down_sampling_method="avg", down_sampling_window=2)
    cfg.__dict__.update(over)
    return cfg


def main():
    G._install_shims()
    TimeMixer = importlib.import_module("models.TimeMixer").TimeMixer
    for name, (B, L, Lp, C, S, P, d, dff, E, k, seed) in FIXTURES.items():
        g = torch.Generator().manual_seed(seed)
        data = torch.randn(B, L, C, generator=g)
        mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
        data = data * mask
        tp = torch.sort(torch.rand(B, L, generator=g), 1).values
        tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
        torch.manual_seed(seed + 2)
        m = TimeMixer(config(C, S, P, d, dff, E, k))
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        m.train()
        out = m.forecasting(tpp, data.clone(), tp, mask)
        up = torch.randn(out.shape, generator=g)
        (out * up).sum().backward()
        arrs = dict(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), out=G._np(out), upstream=G._np(up))
        for key, v in m.state_dict().items():
            if key.endswith(".pe"):
                v = v[:, :S]      # the sinusoid table has 5000 rows; forecasting() reads the first input_len
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
