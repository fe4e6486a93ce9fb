"""Shapes, models and batches shared by tests/test_neuralflow_tanh_ref.py (CPU: the float64 yardstick against the module's composed path)
and tests/test_gpu_neuralflow_tanh.py (GPU: the fused TimeTanh kernels): the smallest shapes at which csrc/neural_flow.hip can still go
wrong with the TimeTanh time net.

  a_defaults     a partial tile of eight windows; two flow layers, so both masks (ordered_0, ordered_1) are taken
  b_tile_edges   nine windows: one full tile and a second workgroup with one window; one channel; three flow layers (odd) and five
                 latents (odd: dim // 2 differs from dim - dim // 2)
  c_envelope     the widths main.py forces (rec_dims 40, latents 20, hidden [32, 32, 32], two flow layers) at C = 64, the channel limit:
                 the largest LDS plan the kernels accept.  (The TimeTanh instance saves no phi tile, so its plan is TimeLinear's.)
  d_dim_one      rec_dims = latents = 1: no coordinate is masked (the module's rule at dim == 1) and the net sees t alone

Times are NOT normalised: observed times are sorted with gaps of 0.05 .. 0.35 and, per window, one gap of 4 .. 7; forecast times follow
the last observed one by up to 8 -- so |scale t| runs from about 0 to well past 2 in both flows and the factor 1 - phi^2 of the
chain rule into time_net.scale is anywhere between 1 and 0 (test_neuralflow_tanh_ref.py asserts that on every case: a kernel that
forgot the factor cannot pass).  Point 1 is unobserved in every window, window 0's last two points are padding (mask and data zero),
and masks are about 70 % ones elsewhere.  `unit=True` divides every time by 16 (into about [0, 1]): the batch for a TimeLinear model,
whose exp(s scale t) is not meant for such spans.

Bars: the project's fp32 bars as tests/ttm_cases.py and tests/informer_cases.py state them -- outputs 1e-4 relative to max, gradients
3e-4 relative to max(|want|, 1e-2 of the largest gradient).  test_neuralflow_tanh_ref.py holds torch's own fp32 CPU run of the
yardstick 4x inside them on every case.  Nothing here comes from the kernel."""
import types

import torch

import neuralflow_tanh_ref as R

OUT_TOL, GRAD_TOL, GRAD_FLOOR = 1e-4, 3e-4, 1e-2
TILE = 8                                              # NF_WT of csrc/neural_flow.hip

SMALL = dict(nf_latents=6, nf_rec_dims=8, nf_hidden_dim=8, nf_hidden_layers=2, nf_flow_layers=2)

# name: (B, L, Lp, C, options)
CASES = {
    "a_defaults": (3, 5, 4, 3, SMALL),
    "b_tile_edges": (TILE + 1, 7, 3, 1, dict(SMALL, nf_flow_layers=3, nf_latents=5)),
    "c_envelope": (8, 3, 2, 64, {}),
    "d_dim_one": (3, 5, 4, 1, dict(SMALL, nf_latents=1, nf_rec_dims=1)),
}


def config(C, L, Lp, device="cpu", **options):
    return types.SimpleNamespace(input_len=L, pred_len=Lp, enc_in=C, device=torch.device(device), **options)


def make_model(dev, case, time_net="TimeTanh", seed=0, **more):
    """the product's NeuralFlow on `dev`, every parameter 0.1 randn off its init, drawn on the CPU"""
    from models.NeuralFlow import NeuralFlow
    B, L, Lp, C, options = case
    torch.manual_seed(2000 + seed)
    m = NeuralFlow(config(C, L, Lp, **dict(options, nf_time_net=time_net, **more)))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
    m.device = torch.device(dev)
    return m.to(dev).train()


def make_batch(dev, case, seed=7, unit=False):
    """-> (tpp (B, Lp), data, tp (B, L), mask, upstream, eps (1, B, latents))"""
    B, L, Lp, C, options = case
    g = torch.Generator().manual_seed(seed)
    gaps = 0.05 + 0.3 * torch.rand(B, L, generator=g)
    long_at = torch.randint(1, L, (B,), generator=g)
    gaps[torch.arange(B), long_at] = 4 + 3 * torch.rand(B, generator=g)
    tp = torch.cumsum(gaps, 1)
    tpp = tp[:, -1:] + torch.cumsum(0.2 + (7.8 / Lp - 0.2) * torch.rand(B, Lp, generator=g), 1)
    if unit:
        tp, tpp = tp / 16, tpp / 16
    data = torch.randn(B, L, C, generator=g)
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    mask[:, 0] = 1
    mask[:, 1] = 0                 # a point no window observes
    mask[0, L - 2:] = 0            # window 0 ends in padding
    up = torch.randn(B, Lp, C, generator=g)
    eps = torch.randn(1, B, options.get("nf_latents", 20), generator=g)
    return tuple(t.to(dev) for t in (tpp, data * mask, tp, mask, up, eps))


def reference(m, batch, dtype=torch.float64):
    """-> (out, name -> gradient or None, stats) of the float64 yardstick on the module's parameters"""
    tpp, data, tp, mask, up, eps = (t.cpu() for t in batch)
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    return R.run(params, tpp, data, tp, mask, eps, up, m.nf_args.time_net, dtype=dtype)


def composed(m, batch):
    """the module's own composed path, as forecasting() runs it below its device and dtype checks, in the dtype of `m` and on its
    device -> (out, name -> gradient or None)"""
    tpp, data, tp, mask, up, eps = batch
    core = m.nf_model_core
    dt = next(m.parameters()).dtype
    tpp, data, tp, mask, up, eps = (t.to(dt) for t in (tpp, data, tp, mask, up, eps))
    m.zero_grad(set_to_none=True)
    B = data.shape[0]
    mu, sigma = core.encoder_z0(torch.cat((data, mask), -1), tp)
    z0 = eps.reshape(B, core.latent_dim) * sigma + mu
    sol_y = core.diffeq_solver(z0.unsqueeze(1).expand(B, tpp.shape[1], core.latent_dim), tpp.unsqueeze(-1))
    out = core.decoder(sol_y)
    (out * up).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def rel(a, b, floor=1e-3):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def grad_errors(got, want):
    """got / want: name -> gradient or None.  -> (the names whose None-ness differs, name -> error relative to max(|want|, 1e-2 of the
    largest gradient))"""
    gmax = max(float(w.abs().max()) for w in want.values() if w is not None)
    diff = sorted(k for k in want if (want[k] is None) != (got[k] is None))
    return diff, {k: rel(got[k], w, floor=GRAD_FLOOR * gmax) for k, w in want.items() if w is not None and got[k] is not None}


def scale_keys(grads):
    return sorted(k for k in grads if k.endswith("time_net.scale"))
