#!/usr/bin/env python3
"""Generate tests/golden/model_cru.npz and model_cru_default.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE): CRU with the
continuous cell at the reference's options, train mode, with every parameter perturbed from its init by 0.1 randn (the bases start at
zero: unperturbed, every transition would be the identity).

    python tests/golden/make_golden_cru.py

    fixture             B  L  Lp  C  lsd  num_basis  bandwidth  hidden
    model_cru           3  6  3   3  8    4          2          16      window 0: two zero-padded trailing points (time 0, mask 0: one step back
                                                                        in time, one standing still); window 1: no observation at all;
                                                                        window 2: an invalid first point
    model_cru_default   2  5  2   5  32   15         3          32      the reference's defaults
    model_cru_rkn       3  6  3   3  8    4          2          16      the discrete cell (cru_rkn) with a time-sensitive coefficient net of one
                                                                        hidden layer (6 units, Tanh); model_cru's batch

History times lie in [0, 1], horizon times in (1, 2], as the collate produces them.  Like make_golden.py it imports the unmodified
reference module at run time and stores tensors only: the inputs, the output, the upstream gradient, the parameters as drawn (`i.`) and
as perturbed (`p.`), every gradient (`g.`), the names without one (`none`, one per line) and the state_dict's keys in order (`keys`):
data, no code."""
import importlib
import types

import numpy as np
import torch

import make_golden as G

FIXTURES = {      # name: (B, L, Lp, C, lsd, num_basis, bandwidth, hidden, seed)
    "model_cru": (3, 6, 3, 3, 8, 4, 2, 16, 71),
    "model_cru_default": (2, 5, 2, 5, 32, 15, 3, 32, 73),
    "model_cru_rkn": (3, 6, 3, 3, 8, 4, 2, 16, 79),
}
RKN = dict(cru_rkn=True, cru_t_sensitive_trans_net=True, cru_trans_net_hidden_units=[6], cru_trans_net_hidden_activation="Tanh")


def config(C, L, Lp, lsd, K, bw, hidden, batch_size=4, device="cpu", **over):
    cfg = types.SimpleNamespace(input_len=L, pred_len=Lp, enc_in=C, batch_size=batch_size, device=torch.device(device), cru_lsd=lsd,
                                cru_num_basis=K, cru_bandwidth=bw, cru_hidden_units=hidden)
    cfg.__dict__.update(over)
    return cfg


def batch(name, B, L, Lp, C, g):
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = 1.0 + torch.sort(torch.rand(B, Lp, generator=g) * 0.999 + 0.001, 1).values
    if name in ("model_cru", "model_cru_rkn"):
        mask[0, 0, 0] = 1
        mask[0, L - 2:] = 0
        tp[0, L - 2:] = 0
        mask[1] = 0
        mask[2, 0] = 0
        mask[2, 1, 1] = 1
    return data * mask, mask, tp, tpp


def main():
    G._install_shims()
    CRU = importlib.import_module("models.CRU").CRU
    for name, (B, L, Lp, C, lsd, K, bw, hidden, seed) in FIXTURES.items():
        g = torch.Generator().manual_seed(seed)
        data, mask, tp, tpp = batch(name, B, L, Lp, C, g)
        torch.manual_seed(seed + 2)
        m = CRU(config(C, L, Lp, lsd, K, bw, hidden, **(RKN if name.endswith("_rkn") else {})))
        arrs = {f"i.{key}": G._np(v).copy() for key, v in m.state_dict().items()}
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        arrs.update({f"p.{key}": G._np(v).copy() for key, v in m.state_dict().items()})
        m.train()
        out = m.forecasting(tpp, data.clone(), tp, mask)
        up = torch.randn(out.shape, generator=g)
        (out * up).sum().backward()
        arrs.update(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), out=G._np(out), upstream=G._np(up))
        none = []
        for key, p in m.named_parameters():
            if p.grad is None:
                none.append(key)
            else:
                arrs[f"g.{key}"] = G._np(p.grad)
        arrs["none"] = np.array("\n".join(none))
        arrs["keys"] = np.array("\n".join(m.state_dict().keys()))
        G.save(name, **arrs)


if __name__ == "__main__":
    main()
