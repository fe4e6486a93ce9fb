#!/usr/bin/env python3
"""Generate tests/golden/model_latentode*.npz from the REAL reference (its checkout at $IMMTSF_REFERENCE): models.LatentODE.LatentODE,
train mode, every parameter perturbed from its init by 0.1 randn (the biases start at zero: a window with no observation would
otherwise sit at exactly 0 through the ODE).

    python tests/golden/make_golden_latentode.py

    fixture                  B  L  Lp  C  latents rec_dims units gru_units
    model_latentode_default  2  5  2   5  20      32       32    32         the reference's defaults
    model_latentode          3  7  4   3  6       8        12    10         span 0.35 < 0.5: the first interval (t[-1] + 0.01 -> t[-1]) takes the
                                                                           RK4 branch; one gap below minimum_step (Euler), one between 1x and 3x
                                                                           (nsub = 2, a single RK4 step), one of 22 grid points; window 1 has no
                                                                           observation at all; point 2 is observed by window 0 only
    model_latentode_span     3  7  4   3  6       8        12    10         span 0.93 > 0.5: the first interval is an Euler step
    model_latentode_L1       3  1  1   3  6       8        12    10         the GRU-only branch; the output is decoder(z0)
    model_latentode_rnn      3  7  4   3  6       8        12    10         ode_z0_encoder = 'rnn'

The one piece of the pipeline that is NOT executed from the real package is torchdiffeq, which is not installed here: the reference's
DiffeqSolver.forward calls `odeint(func, y0, t, method="rk4")` and nothing else of it, and `odeint` below -- this project's own text -- is
that call: one step of the 3/8-rule RK4 (torchdiffeq's rk4_alt_step_func) per interval of the 1-D grid t.

The noise: torch is seeded immediately before forecasting(); afterwards eps is reproduced with the same seed and the reference's own
`Normal(0, 1).sample(size).squeeze(-1)` call, and mu + eps sigma (mu, sigma captured by a hook on the encoder) is asserted to be the
tensor the reference handed to its decoder solver.  Every interval's (prev_t - t_i) / minimum_step is asserted to lie at least 1e-3 away
from every integer and from 1, so a float64 restatement takes the float32 reference's step plan.

Like make_golden.py it imports the unmodified reference module at run time and stores tensors only: the inputs, eps, the output, the
upstream gradient, the parameters as drawn (`i.`) and as perturbed (`p.`), every gradient (`g.`), the names without one (`none`, one per
line) and the state_dict's keys in order (`keys`): data, no code."""
import importlib
import sys
import types

import numpy as np
import torch

import make_golden as G

SMALL = dict(ode_latents=6, ode_rec_dims=8, ode_units=12, ode_gru_units=10)
T7 = [0.10, 0.105, 0.125, 0.20, 0.36, 0.40, 0.45]
T7_WIDE = [0.0, 0.09, 0.2, 0.33, 0.5, 0.71, 0.93]
FIXTURES = {      # name: (B, C, observed times, forecast times, options, seed)
    "model_latentode_default": (2, 5, [0.06, 0.2, 0.3, 0.55, 0.8], [1.1, 1.35], {}, 91),
    "model_latentode": (3, 3, T7, [0.5, 0.58, 0.7, 0.95], SMALL, 93),
    "model_latentode_span": (3, 3, T7_WIDE, [1.02, 1.2, 1.45, 1.5], SMALL, 95),
    "model_latentode_L1": (3, 3, [0.3], [1.2], SMALL, 97),
    "model_latentode_rnn": (3, 3, T7, [0.5, 0.58, 0.7, 0.95], dict(SMALL, ode_z0_encoder="rnn"), 99),
}


def odeint(func, y0, t, method="rk4", **unused):
    """the stand-in for torchdiffeq.odeint (this project's own text, see the module docstring): fixed grid, one 3/8-rule step per interval"""
    assert method == "rk4" and t.dim() == 1
    ys, y = [y0], y0
    for t0, t1 in zip(t[:-1], t[1:]):
        dt = t1 - t0
        k1 = func(t0, y)
        k2 = func(t0 + dt / 3, y + dt * k1 / 3)
        k3 = func(t0 + dt * 2 / 3, y + dt * (k2 - k1 / 3))
        k4 = func(t1, y + dt * (k1 - k2 + k3))
        y = y + (k1 + 3 * (k2 + k3) + k4) * dt * 0.125
        ys.append(y)
    return torch.stack(ys)


def plan_margin(tp):
    """the condition on the observed times (float32, the reference's own operations)"""
    if len(tp) == 1:
        return
    minimum_step = (tp[-1] - tp[0]) / 50
    prev = tp[-1] + 0.01
    for i in reversed(range(len(tp))):
        q = float((prev - tp[i]) / minimum_step)
        assert abs(q - round(q)) >= 1e-3 and abs(q - 1.0) >= 1e-3, (i, q)
        prev = tp[i]


def batch(name, B, C, tp, g):
    L = len(tp)
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    if L > 1:
        mask[:, L // 2, 0] = 1
        mask[1] = 0
        mask[:, 2] = 0
        mask[0, 2, 1] = 1
    return data * mask, mask


def main():
    mod = types.ModuleType("torchdiffeq")
    mod.odeint = odeint
    sys.modules["torchdiffeq"] = mod
    G._install_shims()
    LatentODE = importlib.import_module("models.LatentODE").LatentODE
    for name, (B, C, tp, tpp, options, seed) in FIXTURES.items():
        g = torch.Generator().manual_seed(seed)
        tp, tpp = torch.tensor(tp), torch.tensor(tpp)
        plan_margin(tp)
        data, mask = batch(name, B, C, tp, g)
        torch.manual_seed(seed + 2)
        m = LatentODE(types.SimpleNamespace(C=C, device=torch.device("cpu"), dataset="golden", **options))
        arrs = {f"i.{key}": G._np(v).copy() for key, v in m.state_dict().items()}
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        arrs.update({f"p.{key}": G._np(v).copy() for key, v in m.state_dict().items()})
        m.train()
        core = m.latent_ode_model_core
        seen = {}
        h1 = core.encoder_z0.register_forward_hook(lambda mod_, inp, out: seen.update(mu=out[0].detach(), sigma=out[1].detach()))
        h2 = core.diffeq_solver.register_forward_pre_hook(lambda mod_, inp: seen.update(z0=inp[0].detach()))
        torch.manual_seed(seed + 3)
        out = m.forecasting(tpp, data.clone(), tp, mask)
        h1.remove()
        h2.remove()
        torch.manual_seed(seed + 3)
        eps = torch.distributions.normal.Normal(torch.Tensor([0.]), torch.Tensor([1.])).sample(seen["mu"].size()).squeeze(-1)
        assert torch.equal(seen["mu"] + eps * seen["sigma"], seen["z0"]) or torch.equal(eps * seen["sigma"] + seen["mu"], seen["z0"])
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
