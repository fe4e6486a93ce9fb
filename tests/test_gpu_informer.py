"""Informer's layers on the GPU: the Informer-shaped stack (fused and composed path) against the goldens of the unmodified reference;
immtsf.ops.prob_attention and ConvLayer against the float64 restatement (tests/informer_ref.py, pinned to those goldens in
tests/test_informer_ref.py) at the smallest shapes that reach each branch of the kernels; the tie rule, exact zeros, determinism, the
composed path outside the kernels' limits, and hipGraph capture with the kernel count."""
import copy
import math

import numpy as np
import pytest
import torch

import informer_cases as IC
import informer_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def composed(monkeypatch):
    from immtsf import config
    monkeypatch.setattr(config, "informer_fused", False)


def _run(m, batch):
    m.zero_grad(set_to_none=True)
    out = m.forecasting(*batch[:4])
    (out * batch[4]).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check_model(name, path):
    dev = _dev()
    m, batch, (z, params, none, samples) = IC.golden_model(name, dev)
    torch.manual_seed(int(z["seed"]))
    out, grads = _run(m, batch)
    used = [pa.last_index_sample for pa in m.prob_attentions()]
    assert len(used) == len(samples)
    for got, want in zip(used, samples):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (got, want)
    want_g = {k: (None if k in none else torch.from_numpy(z["g." + k])) for k, _ in m.named_parameters()}
    eo = IC.rel(out, z["out"])
    diff, errs = IC.grad_errors(grads, want_g)
    print(f"{name} [{path}]: out {eo:.2e}, worst gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert eo < IC.OUT_TOL
    assert not diff and max(errs.values()) < IC.GRAD_TOL, (diff, max(errs, key=errs.get))
    state = m.state_dict()
    for k in (k for k in z.files if k.startswith("after.")):
        assert IC.rel(state[k[6:]], z[k]) < IC.OUT_TOL, k


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_fused_stack_meets_the_reference(name):
    _check_model(name, "fused")


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_composed_stack_meets_the_reference(name, composed):
    _check_model(name, "composed")


# ---- prob_attention against the float64 restatement -------------------------------------------------------------------------------------
#       name: (B, H, L_Q, L_K, D, factor, causal, variant)
PA_CASES = {
    "tiny": (1, 2, 3, 3, 4, 1, False, None),
    "all_selected_causal": (2, 2, 4, 4, 8, 5, True, None),
    "causal_query0": (2, 2, 12, 12, 8, 1, True, "force0"),
    "cross": (2, 3, 5, 9, 8, 1, False, None),
    "ref_width": (2, 2, 96, 96, 256, 3, False, None),
    "ref_width_causal": (2, 2, 96, 96, 256, 3, True, None),
    "tile_edges": (1, 2, 130, 67, 68, 2, False, None),
    "unsupported_width": (1, 2, 6, 6, 516, 1, False, "composed"),
    "repeated_keys": (2, 2, 12, 12, 8, 1, False, "repeat"),
}
_pa_cache = {}


def _pa_case(name):
    """inputs on the CPU and the float64 reference (computed once): -> dict.  As in make_golden_informer.py a seed is refused when the
    float64 measure's gap at the cut is below 1e-3 of max|M| -- fp32 (error <= D 2^-24 |M|, 3e-5 at D = 516) cannot then flip the
    selection -- and the next one is tried: the choice looks at the reference alone."""
    if name in _pa_cache:
        return _pa_cache[name]
    B, H, LQ, LK, D, factor, causal, variant = PA_CASES[name]
    U, u = R.n_sample(factor, LK), R.n_sample(factor, LQ)
    scale = 1.0 / math.sqrt(D)
    for attempt in range(20):
        g = torch.Generator().manual_seed(1000 + sorted(PA_CASES).index(name) + 100 * attempt)
        q, k, v = (torch.randn(B, L, H, D, generator=g) for L in (LQ, LK, LK))
        sample = torch.randint(LK, (LQ, U), generator=g).int()
        if variant == "force0":
            q[:, 0] *= 6.0
        if variant == "repeat":
            sample[:, 1] = sample[:, 0]
        up = torch.randn(B, H, LQ, D, generator=g)
        M = R.measure(q.double(), k.double(), sample)
        if R.min_gap(M, u) > 1e-3 and (variant != "force0" or bool((R.select(M, u)[..., 0] == 0).all())):
            break
    else:
        raise AssertionError(f"{name}: no seed with a clear cut")
    c = _pa_reference(q, k, v, sample, u, scale, causal, up)
    _pa_cache[name] = c
    return c


def _pa_reference(q, k, v, sample, u, scale, causal, up, sel=None):
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    out, sel = R.prob_attention(q64, k64, v64, sample, u, scale, causal, sel)
    (out * up.double()).sum().backward()
    gap = R.min_gap(R.measure(q.double(), k.double(), sample), u)
    return dict(q=q, k=k, v=v, sample=sample, u=u, scale=scale, causal=causal, up=up, out=out.detach(), sel=sel, gap=gap,
                grads=dict(q=q64.grad, k=k64.grad, v=v64.grad))


def _pa_gpu(c, dev):
    from immtsf import ops
    q, k, v = (c[n].to(dev).requires_grad_(True) for n in ("q", "k", "v"))
    out, sel = ops.prob_attention(q, k, v, c["sample"].to(dev), c["u"], c["scale"], c["causal"], want_sel=True)
    (out * c["up"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), sel, dict(q=q.grad, k=k.grad, v=v.grad)


def _pa_check(c, out, sel, grads, name):
    assert out.is_contiguous() and tuple(out.shape) == tuple(c["out"].shape)
    assert torch.equal(sel.cpu().long(), c["sel"]), (sel, c["sel"])
    eo = IC.rel(out, c["out"])
    diff, errs = IC.grad_errors(grads, c["grads"])
    print(f"prob_attention {name}: out {eo:.2e}, gradients {errs}")
    assert eo < IC.OUT_TOL and not diff and max(errs.values()) < IC.GRAD_TOL
    unsel = torch.ones(c["q"].shape[0], c["q"].shape[2], c["q"].shape[1], dtype=torch.bool)      # (B, H, L_Q)
    unsel.scatter_(2, c["sel"], False)
    dq = grads["q"].cpu().transpose(1, 2)                                                          # (B, H, L_Q, D)
    assert bool((dq[unsel] == 0).all()), "unselected rows of dq must be exact zeros"


@pytest.mark.parametrize("name", sorted(PA_CASES))
def test_prob_attention_matches_float64(name):
    dev = _dev()
    from immtsf import ops
    B, H, LQ, LK, D, factor, causal, variant = PA_CASES[name]
    c = _pa_case(name)
    assert ops.prob_attention_supported(LQ, LK, D, c["u"]) == (variant != "composed")
    out, sel, grads = _pa_gpu(c, dev)
    _pa_check(c, out, sel, grads, name)
    out2, sel2, grads2 = _pa_gpu(c, dev)      # two runs: the same bits
    assert torch.equal(out, out2) and torch.equal(sel, sel2) and all(torch.equal(grads[n], grads2[n]) for n in grads)


@pytest.mark.parametrize("name", ["cross", "causal_query0", "ref_width_causal"])
def test_prob_attention_composed_path_matches_float64(name, composed):
    c = _pa_case(name)
    out, sel, grads = _pa_gpu(c, _dev())
    _pa_check(c, out, sel, grads, name + " [composed]")


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_a_tie_at_the_cut_goes_to_the_lower_index(path, monkeypatch):
    """two identical query rows with identical samples have the same measure bit for bit; placed so that they compete for the last
    selected slot, the lower index must win, whichever of the two it is"""
    dev = _dev()
    from immtsf import config
    monkeypatch.setattr(config, "informer_fused", path == "fused")
    B, H, L, D, factor = 1, 1, 12, 8, 1
    g = torch.Generator().manual_seed(77)
    q, k, v = (torch.randn(B, L, H, D, generator=g) for _ in range(3))
    up = torch.randn(B, H, L, D, generator=g)
    U, u = R.n_sample(factor, L), R.n_sample(factor, L)
    sample = torch.randint(L, (L, U), generator=g).int()
    order = torch.sort(R.measure(q.double(), k.double(), sample)[0, 0], descending=True).indices.tolist()
    last, losers = order[u - 1], order[u:]
    for other in (min(losers), max(losers)):      # one twin below `last` or above it, as the draw has it; both orders over the two picks
        q2, s2 = q.clone(), sample.clone()
        q2[:, other], s2[other] = q[:, last], sample[last]
        M = R.measure(q2.double(), k.double(), s2)[0, 0]
        assert M[other] == M[last]
        want = R.select(M[None, None], u)
        assert min(other, last) in want[0, 0].tolist() and max(other, last) not in want[0, 0].tolist()
        c = _pa_reference(q2, k, v, s2, u, 1.0 / math.sqrt(D), False, up, sel=want)
        out, sel, grads = _pa_gpu(c, dev)
        _pa_check(c, out, sel, grads, f"tie {last}/{other} [{path}]")


# ---- ConvLayer ---------------------------------------------------------------------------------------------------------------------------
def _conv_module(params, dev):
    from layers.Transformer_EncDec import ConvLayer
    m = ConvLayer(params["downConv.weight"].shape[0])
    m.load_state_dict(params, strict=True)
    return m.to(dev)


def _conv_run(m, x, up, mode):
    m.train(mode == "train")
    m.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    out = m(xi)
    (out * up).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), {**{k: p.grad for k, p in m.named_parameters()}, "x": xi.grad}


def _conv_want_grads(want, mode, got):
    if mode == "train":      # zero analytically under batch statistics: rounding noise on either side (test_informer_ref.py)
        gmax = max(float(w.abs().max()) for w in want.values())
        assert float(got["downConv.bias"].abs().max()) < 1e-4 * gmax
        want = {k: w for k, w in want.items() if k != "downConv.bias"}
    return want


@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("case", sorted(IC.CONV_CASES))
def test_conv_layer_meets_the_reference(case, path, monkeypatch):
    dev = _dev()
    from immtsf import config
    monkeypatch.setattr(config, "informer_fused", path == "fused")
    z = np.load(IC.GOLDEN + "/layer_conv_distil.npz")
    m = _conv_module(IC.conv_params(z, case), dev)
    x = torch.from_numpy(z[f"{case}.x"]).to(dev)
    for mode in ("eval", "train"):      # the fixture's order: the evaluation call sees the buffers before the training call
        out, grads = _conv_run(m, x, torch.from_numpy(z[f"{case}.{mode}.upstream"]).to(dev), mode)
        want = {k: torch.from_numpy(z[f"{case}.{mode}.g.{k}"]) for k in ("downConv.weight", "downConv.bias", "norm.weight", "norm.bias")}
        want["x"] = torch.from_numpy(z[f"{case}.{mode}.gx"])
        eo = IC.rel(out, z[f"{case}.{mode}.out"])
        diff, errs = IC.grad_errors(grads, _conv_want_grads(want, mode, grads))
        print(f"ConvLayer {case} {mode} [{path}]: out {eo:.2e}, gradients {errs}")
        assert eo < IC.OUT_TOL and not diff and max(errs.values()) < IC.GRAD_TOL
    state = m.state_dict()
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert IC.rel(state["norm." + k], z[f"{case}.after.norm.{k}"]) < IC.OUT_TOL, k
    assert int(state["norm.num_batches_tracked"]) == 1


CONV_SHAPES = {"odd_rows": (2, 3, 8, True), "wide": (2, 8, 512, True), "unsupported_width": (2, 5, 6, False)}


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("name", sorted(CONV_SHAPES))
def test_conv_layer_matches_float64(name, mode):
    dev = _dev()
    from immtsf import ops
    from layers.Transformer_EncDec import ConvLayer
    B, L, d, kernel = CONV_SHAPES[name]
    assert ops.conv_distil_supported(d) == kernel
    g = torch.Generator().manual_seed(300 + d + L)
    torch.manual_seed(5)
    m = ConvLayer(d)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        m.norm.running_mean.copy_(0.1 * torch.randn(d, generator=g))
        m.norm.running_var.copy_(1 + 0.2 * torch.rand(d, generator=g))
    x, up = torch.randn(B, L, d, generator=g), torch.randn(B, (L + 1) // 2 + 1, d, generator=g)
    p64 = {k: (t.double().requires_grad_(True) if t.is_floating_point() else t.clone()) for k, t in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    want_out, after = R.conv_layer(x64, p64, "", mode == "train")
    (want_out * up.double()).sum().backward()
    m = m.to(dev)
    out, grads = _conv_run(m, x.to(dev), up.to(dev), mode)
    want = {k: p64[k].grad for k in ("downConv.weight", "downConv.bias", "norm.weight", "norm.bias")}
    want["x"] = x64.grad
    eo = IC.rel(out, want_out)
    diff, errs = IC.grad_errors(grads, _conv_want_grads(want, mode, grads))
    print(f"ConvLayer {name} {mode}: out {eo:.2e}, gradients {errs}")
    assert eo < IC.OUT_TOL and not diff and max(errs.values()) < IC.GRAD_TOL
    state = m.state_dict()
    for k, w in after.items():
        assert IC.rel(state["norm." + k], w) < IC.OUT_TOL, k


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
def _capture(m, static):
    from immtsf import step_plan
    dev = static[0].device
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(m, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    step_plan.collect_before_capture()
    with torch.cuda.graph(graph):
        out = m.forecasting(*static[:4])
        (out * static[4]).sum().backward()
    return graph, out


def _kernels_of_a_step(m, static):
    """the device kernels of one forward + backward, by name.  Counted on an eager run of exactly the step that is captured (the same
    modules, knobs and device-resident samples, so the same launches as the graph's kernel nodes): torch's profiler does not trace the
    kernels of a replayed hipGraph."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        _run(m, static)
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset"))]


def test_forward_backward_under_graph_capture():
    """forward + backward of the small model captured on one stream.  With sample_override (on the device) two replays give the eager
    run's numbers (the GEMMs' weight gradients are split-K sums, so to 1e-5 rather than bit for bit); without it the samples are drawn
    on the device inside the graph.  The fused graph holds fewer kernels than the composed one."""
    dev = _dev()
    from immtsf import config
    m, batch, (z, _, _, samples) = IC.golden_model("model_informer", dev)
    static = tuple(t.clone() for t in batch)
    for pa, s in zip(m.prob_attentions(), samples):
        pa.sample_override = s.to(dev)
    want_out, want_g = _run(copy.deepcopy(m), batch)
    graph, out = _capture(m, static)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert IC.rel(out, want_out) < 1e-5
        diff, errs = IC.grad_errors({k: p.grad for k, p in m.named_parameters()}, want_g)
        assert not diff and max(errs.values()) < 1e-5, errs
    n_fused = len(_kernels_of_a_step(m, static))
    del graph

    m2, _, _ = IC.golden_model("model_informer", dev)
    graph2, out2 = _capture(m2, static)
    for _ in range(2):
        graph2.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out2).all()) and all(bool(torch.isfinite(p.grad).all()) for p in m2.parameters() if p.grad is not None)
    for pa in m2.prob_attentions():
        assert pa.last_index_sample.is_cuda and pa.last_index_sample.dtype == torch.int32
    del graph2

    config.informer_fused = False
    try:
        m3, _, _ = IC.golden_model("model_informer", dev)
        for pa, s in zip(m3.prob_attentions(), samples):
            pa.sample_override = s.to(dev)
        graph3, out3 = _capture(m3, static)
        graph3.replay()
        torch.cuda.synchronize()
        assert IC.rel(out3, want_out) < 1e-5
        n_composed = len(_kernels_of_a_step(m3, static))
    finally:
        config.informer_fused = True
    print(f"kernels per replayed forward + backward: fused {n_fused}, composed {n_composed}")
    assert 0 < n_fused < n_composed
