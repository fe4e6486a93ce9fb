#!/usr/bin/env python3
"""Generate tests/golden/model_neuralflow*.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE): models.NeuralFlow.NeuralFlow,
train mode, every parameter perturbed from its init by 0.1 randn (transform_z0's and the decoder's biases start at zero).

    python tests/golden/make_golden_neuralflow.py

    fixture                     B  L  Lp  C  latents rec_dims hidden      time net
    model_neuralflow_default    2  5  2   5  20      40       [32,32,32]  TimeLinear   the reference's defaults; one time axis for both windows
    model_neuralflow            3  7  4   3  6       8        [12,12]     TimeLinear   every window has its own times; window 1 has no
                                                                                      observation at all; point 2 is observed by window 0 only
    model_neuralflow_L1         3  1  1   3  6       8        [12,12]     TimeLinear   one observed point, one forecast time
    model_neuralflow_tanh       3  7  4   3  6       8        [12,12]     TimeTanh

The one piece of the pipeline that is NOT executed from the real package is `stribor`, which is not installed here.  The reference's
models/flow.py takes from it ContinuousAffineCoupling, Flow, net.MLP and the time nets; the stand-ins below -- this project's own text --
implement the published definition of the continuous affine coupling layer (Bilos et al., "Neural Flows", 2021) as stribor 0.1.0 is
remembered to: mask = ordered_{0,1} / none, (s, b) = latent_net(cat(x m, t)), (phi_s, phi_b) = time_net(t), y = x exp(s phi_s) + b phi_b,
out = y (1 - m) + x m; MLP with Tanh between its Linears in `net`; TimeLinear / TimeTanh with one parameter `scale` (1, out_dim),
xavier_uniform_.  THIS COULD NOT BE CHECKED AGAINST THE PACKAGE.  Everything else is the reference's own code: the encoder and its LSTM
cell, SolverWrapper's reshapes, CouplingFlow, get_reconstruction, the sampling call, the decoder.  (`torchdiffeq` is a stub too:
lib/neural_flow_components/models/ode.py imports `odeint_adjoint` from it and the flow model never calls it.)

The noise: torch is seeded immediately before forecasting(); afterwards eps is reproduced with the same seed and the reference's own
`Normal(0, 1).sample(size).squeeze(-1)` call, and eps sigma + mu (mu, sigma captured by a hook on the encoder) is asserted to be the
tensor the reference handed to its decode solver.

Like make_golden.py it imports the unmodified reference module at run time and stores tensors only: the inputs, eps, the output, the
upstream gradient, the parameters as drawn (`i.`) and as perturbed (`p.`), every gradient (`g.`), the names without one (`none`, one per
line) and the state_dict's keys in order (`keys`): data, no code."""
import importlib
import sys
import types

import numpy as np
import torch
import torch.nn as nn

import make_golden as G

SMALL = dict(nf_latents=6, nf_rec_dims=8, nf_hidden_dim=12, nf_hidden_layers=2)
FIXTURES = {      # name: (B, C, L, Lp, every window its own times, options, seed)
    "model_neuralflow_default": (2, 5, 5, 2, False, {}, 191),
    "model_neuralflow": (3, 3, 7, 4, True, SMALL, 193),
    "model_neuralflow_L1": (3, 3, 1, 1, True, SMALL, 195),
    "model_neuralflow_tanh": (3, 3, 7, 4, True, dict(SMALL, nf_time_net="TimeTanh"), 197),
}


# ---- the stand-in for stribor (this project's own text, see the module docstring)
class MLP(nn.Module):
    def __init__(self, in_dim, hidden_dims, out_dim, activation="Tanh", final_activation=None):
        super().__init__()
        assert activation == "Tanh" and final_activation in (None, "Identity")
        dims = [in_dim] + list(hidden_dims) + [out_dim]
        layers = []
        for a, b in zip(dims[:-1], dims[1:]):
            layers += [nn.Linear(a, b), nn.Tanh()]
        self.net = nn.Sequential(*layers[:-1])

    def forward(self, x):
        return self.net(x)


class TimeLinear(nn.Module):
    def __init__(self, out_dim, hidden_dim=None):
        super().__init__()
        self.scale = nn.Parameter(torch.empty(1, out_dim))
        nn.init.xavier_uniform_(self.scale)

    def forward(self, t):
        return self.scale * t


class TimeTanh(TimeLinear):
    def forward(self, t):
        return torch.tanh(self.scale * t)


def get_mask(name, dim):
    if name == "none":
        return torch.zeros(dim)
    assert name in ("ordered_0", "ordered_1")
    m = torch.zeros(dim)
    m[:dim // 2] = 1
    return m if name == "ordered_0" else 1 - m


class ContinuousAffineCoupling(nn.Module):
    def __init__(self, latent_net, time_net, mask):
        super().__init__()
        self.latent_net = latent_net
        self.time_net = time_net
        self.mask_name = mask

    def forward(self, x, t):
        m = get_mask(self.mask_name, x.shape[-1]).to(x)
        s, b = self.latent_net(torch.cat((x * m, t), -1)).chunk(2, -1)
        phi_s, phi_b = self.time_net(t).chunk(2, -1)
        y = x * torch.exp(s * phi_s) + b * phi_b
        return y * (1 - m) + x * m, (s * phi_s) * (1 - m)


class Flow(nn.Module):
    def __init__(self, transforms):
        super().__init__()
        self.transforms = nn.ModuleList(transforms)

    def forward(self, x, t=None):
        ljd = 0
        for f in self.transforms:
            x, d = f(x, t)
            ljd = ljd + d
        return x, ljd


def install_stribor():
    st = types.ModuleType("stribor")
    st.net = types.ModuleType("stribor.net")
    st.net.MLP, st.net.TimeLinear, st.net.TimeTanh = MLP, TimeLinear, TimeTanh
    st.ContinuousAffineCoupling, st.Flow = ContinuousAffineCoupling, Flow
    sys.modules["stribor"], sys.modules["stribor.net"] = st, st.net
    td = types.ModuleType("torchdiffeq")

    def odeint_adjoint(*a, **k):
        raise RuntimeError("the flow model calls no ODE solver")
    td.odeint_adjoint = td.odeint = odeint_adjoint
    sys.modules["torchdiffeq"] = td


def batch(B, C, L, Lp, own_times, g):
    """times in [0, 1]: observed in [0, 0.6], forecast in [0.62, 1], increasing per window"""
    rows = B if own_times else 1
    tp = torch.sort(torch.rand(rows, L, generator=g) * 0.6, dim=1).values.expand(B, L).contiguous()
    tpp = (0.62 + torch.sort(torch.rand(rows, Lp, generator=g) * 0.38, dim=1).values).expand(B, Lp).contiguous()
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    if L > 2:
        mask[:, L // 2, 0] = 1
        mask[1] = 0
        mask[:, 2] = 0
        mask[0, 2, 1] = 1
    return tp, tpp, data * mask, mask


def main():
    install_stribor()
    G._install_shims()
    NeuralFlow = importlib.import_module("models.NeuralFlow").NeuralFlow
    assert "neural_flow_components" in sys.modules["models.NeuralFlow"].create_LatentODE_model.__module__
    for name, (B, C, L, Lp, own_times, options, seed) in FIXTURES.items():
        g = torch.Generator().manual_seed(seed)
        tp, tpp, data, mask = batch(B, C, L, Lp, own_times, g)
        torch.manual_seed(seed + 2)
        m = NeuralFlow(types.SimpleNamespace(input_len=L, pred_len=Lp, enc_in=C, device=torch.device("cpu"), **options))
        arrs = {f"i.{key}": G._np(v).copy() for key, v in m.state_dict().items()}
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        arrs.update({f"p.{key}": G._np(v).copy() for key, v in m.state_dict().items()})
        m.train()
        core = m.nf_model_core
        seen = {}
        h1 = core.encoder_z0.register_forward_hook(lambda mod_, inp, out: seen.update(mu=out[0].detach(), sigma=out[1].detach()))
        h2 = core.diffeq_solver.register_forward_pre_hook(lambda mod_, inp: seen.update(z0=inp[0].detach()))
        torch.manual_seed(seed + 3)
        out = m.forecasting(tpp, data.clone(), tp, mask)
        h1.remove()
        h2.remove()
        assert tuple(out.shape) == (B, Lp, C) and tuple(seen["z0"].shape) == (1, B, 1, core.latent_dim)
        torch.manual_seed(seed + 3)
        eps = torch.distributions.normal.Normal(torch.Tensor([0.]), torch.Tensor([1.])).sample(seen["mu"].size()).squeeze(-1)
        assert torch.equal(eps * seen["sigma"] + seen["mu"], seen["z0"].squeeze(-2))
        up = torch.randn(out.shape, generator=g)
        (out * up).sum().backward()
        arrs.update(data=G._np(data), mask=G._np(mask), tp=G._np(tp), tpp=G._np(tpp), eps=G._np(eps[0]), out=G._np(out), upstream=G._np(up))
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
