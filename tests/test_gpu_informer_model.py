"""models.Informer of this build on the GPU: the whole model (fused stages and composed path) against the goldens of the unmodified
reference and, at full lengths, against the float64 restatement (tests/informer_ref.py); the two stages of csrc/informer.hip against
their float64 restatements (tests/informer_model_ref.py, pinned in tests/test_informer_model_ref.py) at the smallest shapes that reach
each branch of the kernels, with the exact zeros, determinism, the dropout masks, and hipGraph capture with the kernel count."""
import copy

import pytest
import torch

import informer_cases as IC
import informer_model_ref as MR
import informer_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def composed(monkeypatch):
    from immtsf import config
    monkeypatch.setattr(config, "informer_model_fused", False)


def _run(m, batch):
    m.zero_grad(set_to_none=True)
    out = m.forecasting(*batch[:4])
    (out * batch[4]).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _golden_model(name, dev, **over):
    """models.Informer with the fixture's state, in train mode on `dev`; -> (module, (tpp, data, tp, mask, upstream), golden)"""
    from models.Informer import Informer
    z, params, none, samples = IC.golden(name)
    m = Informer(IC.config(IC.FIXTURES[name], device=str(dev), **over))
    m.load_state_dict(params, strict=True)
    m = m.to(dev).train()
    batch = tuple(torch.from_numpy(z[k]).to(dev) for k in ("tpp", "data", "tp", "mask", "upstream"))
    return m, batch, (z, params, none, samples)


# ---- 1. the whole model against the goldens ---------------------------------------------------------------------------------------------
def _check_model(name, path):
    dev = _dev()
    m, batch, (z, params, none, samples) = _golden_model(name, dev)
    torch.manual_seed(int(z["seed"]))
    out, grads = _run(m, batch)
    assert m.fused_calls == (1 if path == "fused" else 0)
    used = [pa.last_index_sample for pa in m.prob_attentions()]
    assert len(used) == len(samples)
    for got, want in zip(used, samples):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (got, want)
    want_g = {k: (None if k in none else torch.from_numpy(z["g." + k])) for k, _ in m.named_parameters()}
    eo = IC.rel(out, z["out"])
    diff, errs = IC.grad_errors(grads, want_g)
    print(f"{name} [{path}]: out {eo:.2e}, worst gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert out.is_contiguous() and eo < IC.OUT_TOL
    assert not diff and max(errs.values()) < IC.GRAD_TOL, (diff, max(errs, key=errs.get))
    state = m.state_dict()
    for k in (k for k in z.files if k.startswith("after.")):
        assert IC.rel(state[k[6:]], z[k]) < IC.OUT_TOL, k


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_fused_model_meets_the_reference(name):
    _check_model(name, "fused")


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_composed_model_meets_the_reference(name, composed):
    _check_model(name, "composed")


# ---- 2. the whole model against float64 where the goldens do not reach ----------------------------------------------------------------------
def _sample_shapes(opts, S, P):
    """(L_Q, U_part) of every ProbAttention call, in call order"""
    f, shapes, Ls = opts["factor"], [], S
    for i in range(opts["e_layers"]):
        shapes.append((Ls, R.n_sample(f, Ls), Ls))
        if opts["distil"] and i < opts["e_layers"] - 1:
            Ls = (Ls + 1) // 2 + 1
    for _ in range(opts["d_layers"]):
        shapes += [(P, R.n_sample(f, P), P), (P, R.n_sample(f, Ls), Ls)]
    return shapes


_model_cache = {}


def _model_case(key, opts, B, L, Lp, golden_name=None):
    """a module on the CPU (the fixture's state, or its own seeded initial state), seeded inputs and samples, and the float64 reference
    (computed once): -> dict.  As _pa_case of test_gpu_informer.py a seed is refused when the float64 measure's gap at a cut is below
    1e-3 of max|M| in any ProbAttention call, and the next one is tried: the choice looks at the reference alone."""
    if key in _model_cache:
        return _model_cache[key]
    from models.Informer import Informer
    torch.manual_seed(11)
    m = Informer(IC.config(opts, batch_size=B))
    if golden_name is not None:
        m.load_state_dict(IC.golden(golden_name)[1], strict=True)
    S, P, C = opts["input_len"], opts["pred_len"], opts["C"]
    p64 = {k: (v.detach().double().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()}
    for attempt in range(20):
        g = torch.Generator().manual_seed(4000 + 100 * attempt + len(key))
        data = torch.randn(B, L, C, generator=g)
        mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
        tp = torch.sort(torch.rand(B, L, generator=g), 1).values
        tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
        up = torch.randn(B, Lp, opts["c_out"], generator=g)
        samples = [torch.randint(LK, (LQ, U), generator=g).int() for LQ, U, LK in _sample_shapes(opts, S, P)]
        for t in p64.values():
            if t.is_floating_point():
                t.grad = None
        out, _, log = R.informer(p64, opts, tpp.double(), data.double(), tp.double(), mask.double(), samples)
        if min(log) > 1e-3:
            break
    else:
        raise AssertionError(f"{key}: no seed with a clear cut in 20")
    (out * up.double()).sum().backward()
    names = [k for k, _ in m.named_parameters()]
    c = dict(module=m, batch=(tpp, data, tp, mask, up), samples=samples, out=out.detach(), gap=min(log),
             grads={k: (None if p64[k].grad is None else p64[k].grad.clone()) for k in names})
    _model_cache[key] = c
    return c


def _check_against_float64(c, dev, want_fused, label):
    m = copy.deepcopy(c["module"]).to(dev).train()
    m.zeros_pad = m.zeros_pad.to(dev)
    for pa, s in zip(m.prob_attentions(), c["samples"]):
        pa.sample_override = s.to(dev)
    out, grads = _run(m, tuple(t.to(dev) for t in c["batch"]))
    assert m.fused_calls == (1 if want_fused else 0)
    eo = IC.rel(out, c["out"])
    diff, errs = IC.grad_errors(grads, c["grads"])
    print(f"{label}: gap {c['gap']:.1e}, out {eo:.2e}, worst gradient {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert eo < IC.OUT_TOL
    assert not diff and max(errs.values()) < IC.GRAD_TOL, (diff, max(errs, key=errs.get))


@pytest.mark.parametrize("path", ["fused", "composed"])
def test_model_at_full_lengths_matches_float64(path, monkeypatch):
    """L == input_len and Lp == pred_len: no padding on either side, which neither golden reaches"""
    from immtsf import config
    monkeypatch.setattr(config, "informer_model_fused", path == "fused")
    opts = IC.FIXTURES["model_informer"]
    c = _model_case("full", opts, 1, opts["input_len"], opts["pred_len"], golden_name="model_informer")
    _check_against_float64(c, _dev(), path == "fused", f"full lengths [{path}]")


def test_unsupported_width_takes_the_composed_path():
    from immtsf import ops
    opts = dict(IC.FIXTURES["model_informer"], d_model=516)
    assert not ops.informer_model_supported(opts["input_len"], opts["pred_len"], opts["C"], 516)
    c = _model_case("w516", opts, 1, 10, 4)
    _check_against_float64(c, _dev(), False, "d_model 516 [composed]")


# ---- 3. the front stage against float64 -----------------------------------------------------------------------------------------------------
#        name: (B, L, input_len, Lp, pred_len, C, d_model)
FRONT_CASES = {
    "tiny": (1, 1, 2, 1, 1, 1, 4),                 # input_len 2: taps l-1 and l+1 are the same row; pred_len 1: all three taps one element
    "golden": (3, 10, 12, 4, 5, 3, 16),            # the fixtures' shape; an unobserved window, a channel observed once
    "full": (2, 12, 12, 5, 5, 3, 16),              # no padding on either side
    "odd": (2, 100, 130, 3, 7, 16, 68),            # 33 channels; a width that is no multiple of 64; 9 row tiles, the last one cut
    "ref_width": (2, 96, 96, 24, 24, 7, 512),      # the reference's width
    "widest": (1, 3, 4, 2, 3, 32, 1024),           # the limits of C and d_model: 65 channels, 17 per channel group; 16 column tiles
}
_front_cache = {}


def _front_case(name, p=0.0, scales=None):
    """inputs on the CPU and the float64 reference -> dict (cached per name when there is no dropout)"""
    if scales is None and name in _front_cache:
        return _front_cache[name]
    B, L, S, Lp, P, C, D = FRONT_CASES[name]
    g = torch.Generator().manual_seed(7000 + sorted(FRONT_CASES).index(name))
    data = torch.randn(B, L, C, generator=g) * 2 + 1
    mask = (torch.rand(B, L, C, generator=g) < 0.7).float()
    if name == "golden":
        mask[1] = 0                                  # cnt clamps to 1, stdev = sqrt(1e-5)
        mask[0, :, 2] = 0
        mask[0, 3, 2] = 1                            # observed exactly once: var 0
    tp = torch.sort(torch.rand(B, L, generator=g), 1).values
    tpp = torch.sort(torch.rand(B, Lp, generator=g), 1).values
    W_enc, W_dec = (torch.randn(D, 2 * C + 1, 3, generator=g) * 0.3 for _ in range(2))
    pe_enc, pe_dec = (torch.randn(max(S, P) + 3, D, generator=g) for _ in range(2))
    up_e, up_d = torch.randn(B, S, D, generator=g), torch.randn(B, P, D, generator=g)
    We, Wd = W_enc.double().requires_grad_(True), W_dec.double().requires_grad_(True)
    se, sd = (None, None) if scales is None else (scales[0].double(), scales[1].double())
    enc, dec, means, stdev = MR.front(data.double(), mask.double(), tp.double(), tpp.double(), S, P, We, Wd, pe_enc.double(), pe_dec.double(),
                                      se, sd)
    ((enc * up_e.double()).sum() + (dec * up_d.double()).sum()).backward()
    c = dict(batch=(data, mask, tp, tpp), W=(W_enc, W_dec), pe=(pe_enc, pe_dec), up=(up_e, up_d), dims=(S, P),
             want=dict(enc=enc.detach(), dec=dec.detach(), means=means, stdev=stdev), grads=dict(W_enc=We.grad, W_dec=Wd.grad))
    if scales is None:
        _front_cache[name] = c
    return c


def _front_gpu(c, dev, p=0.0, training=False, seed=None):
    from immtsf import ops
    data, mask, tp, tpp = (t.to(dev) for t in c["batch"])
    W_enc, W_dec = (t.to(dev).requires_grad_(True) for t in c["W"])
    pe_enc, pe_dec = (t.to(dev) for t in c["pe"])
    enc, dec, means, stdev = ops.informer_front(data, mask, tp, tpp, *c["dims"], W_enc, W_dec, pe_enc, pe_dec, p, training, seed)
    ((enc * c["up"][0].to(dev)).sum() + (dec * c["up"][1].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return dict(enc=enc.detach(), dec=dec.detach(), means=means, stdev=stdev), dict(W_enc=W_enc.grad, W_dec=W_dec.grad)


def _front_check(c, out, grads, label):
    errs_o = {k: IC.rel(out[k], w) for k, w in c["want"].items()}
    diff, errs = IC.grad_errors(grads, c["grads"])
    print(f"informer_front {label}: outputs {errs_o}, gradients {errs}")
    assert max(errs_o.values()) < IC.OUT_TOL and not diff and max(errs.values()) < IC.GRAD_TOL


@pytest.mark.parametrize("name", sorted(FRONT_CASES))
def test_front_matches_float64(name):
    dev = _dev()
    from immtsf import ops
    B, L, S, Lp, P, C, D = FRONT_CASES[name]
    assert ops.informer_model_supported(S, P, C, D)
    c = _front_case(name)
    out, grads = _front_gpu(c, dev)
    assert tuple(out["enc"].shape) == (B, S, D) and tuple(out["dec"].shape) == (B, P, D) and tuple(out["means"].shape) == (B, 1, C)
    _front_check(c, out, grads, name)
    assert bool((grads["W_dec"][:, :2 * C, :] == 0).all()), "dW_dec outside the time channel must be exact zeros"
    out2, grads2 = _front_gpu(c, dev)      # two runs: the same bits
    assert all(torch.equal(out[k], out2[k]) for k in out) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    if name == "golden":
        floor = 1e-5 ** 0.5      # the unobserved window (cnt clamps to 1) and the channel observed once (var 0): stdev = sqrt(1e-5)
        assert bool((out["means"][1] == 0).all()) and float((out["stdev"][1] - floor).abs().max()) < 1e-6 * floor
        assert abs(float(out["stdev"][0, 0, 2]) - floor) < 1e-6 * floor


# ---- 4. the tail stage against float64 ------------------------------------------------------------------------------------------------------
#        (B, Lp, pred_len, d_model, C)
TAIL_CASES = {"tiny": (1, 1, 1, 4, 1), "golden": (3, 4, 5, 16, 3), "odd": (2, 3, 7, 68, 16), "ref_width": (2, 24, 24, 512, 7),
              "widest": (1, 2, 3, 1024, 32), "slices": (3, 50, 50, 64, 5)}      # slices: 150 rows = three slices of the backward
_tail_cache = {}


def _tail_case(name):
    if name in _tail_cache:
        return _tail_cache[name]
    B, Lp, P, D, C = TAIL_CASES[name]
    g = torch.Generator().manual_seed(8000 + sorted(TAIL_CASES).index(name))
    x = torch.randn(B, P, D, generator=g) * 1.5 + 0.3
    t = dict(gamma=1 + 0.2 * torch.randn(D, generator=g), beta=0.2 * torch.randn(D, generator=g),
             W=torch.randn(C, D, generator=g) / D ** 0.5, b=0.3 * torch.randn(C, generator=g))
    means, stdev = torch.randn(B, 1, C, generator=g), 0.2 + torch.rand(B, 1, C, generator=g)
    up = torch.randn(B, Lp, C, generator=g)
    leaves = {k: v.double().requires_grad_(True) for k, v in dict(t, x=x).items()}
    y = MR.tail(leaves["x"], leaves["gamma"], leaves["beta"], leaves["W"], leaves["b"], means.double(), stdev.double(), Lp)
    (y * up.double()).sum().backward()
    c = dict(x=x, params=t, means=means, stdev=stdev, up=up, Lp=Lp, out=y.detach(), grads={k: v.grad for k, v in leaves.items()})
    _tail_cache[name] = c
    return c


def _tail_gpu(c, dev):
    from immtsf import ops
    D, C = c["x"].shape[-1], c["params"]["W"].shape[0]
    norm, proj = torch.nn.LayerNorm(D), torch.nn.Linear(D, C)
    with torch.no_grad():
        norm.weight.copy_(c["params"]["gamma"]), norm.bias.copy_(c["params"]["beta"])
        proj.weight.copy_(c["params"]["W"]), proj.bias.copy_(c["params"]["b"])
    norm, proj = norm.to(dev), proj.to(dev)
    x = c["x"].to(dev).requires_grad_(True)
    y = ops.informer_tail(x, norm, proj, c["means"].to(dev), c["stdev"].to(dev), c["Lp"])
    (y * c["up"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), dict(x=x.grad, gamma=norm.weight.grad, beta=norm.bias.grad, W=proj.weight.grad, b=proj.bias.grad)


@pytest.mark.parametrize("name", sorted(TAIL_CASES))
def test_tail_matches_float64(name):
    dev = _dev()
    B, Lp, P, D, C = TAIL_CASES[name]
    c = _tail_case(name)
    y, grads = _tail_gpu(c, dev)
    assert y.is_contiguous() and tuple(y.shape) == (B, Lp, C)
    eo = IC.rel(y, c["out"])
    diff, errs = IC.grad_errors(grads, c["grads"])
    print(f"informer_tail {name}: out {eo:.2e}, gradients {errs}")
    assert eo < IC.OUT_TOL and not diff and max(errs.values()) < IC.GRAD_TOL
    assert tuple(grads["x"].shape) == (B, P, D) and bool((grads["x"][:, Lp:] == 0).all()), "dx rows t >= Lp must be exact zeros"
    y2, grads2 = _tail_gpu(c, dev)      # two runs: the same bits
    assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 5. dropout -----------------------------------------------------------------------------------------------------------------------------
def test_front_dropout_masks_are_the_philox_sites(monkeypatch):
    dev = _dev()
    from immtsf import config, ops
    monkeypatch.setattr(config, "_device_counters", {})      # the key is the seed alone
    B, L, S, Lp, P, C, D = FRONT_CASES["golden"]
    p, seed = 0.25, 0x1234_5678_9ABC
    c0 = _front_case("golden")
    plain, _ = _front_gpu(c0, dev)
    keep_e = ops.dropout_keep_mask(seed, ops.SITE_INFORMER_ENC, B * S * D, p, dev)
    keep_d = ops.dropout_keep_mask(seed, ops.SITE_INFORMER_DEC, B * P * D, p, dev)
    torch.cuda.synchronize()
    assert 0.6 < float(keep_e.float().mean()) < 0.9 and 0.5 < float(keep_d.float().mean()) < 0.95
    assert not torch.equal(keep_d, keep_e[:B * P * D]), "the two embeddings must draw from distinct sites"
    se, sd = keep_e.float().view(B, S, D) / (1 - p), keep_d.float().view(B, P, D) / (1 - p)
    c = _front_case("golden", p, (se.cpu(), sd.cpu()))
    out, grads = _front_gpu(c, dev, p, True, seed)
    assert float((out["enc"] - plain["enc"] * se).abs().max()) <= 1e-6 * float(plain["enc"].abs().max())
    assert float((out["dec"] - plain["dec"] * sd).abs().max()) <= 1e-6 * float(plain["dec"].abs().max())
    _front_check(c, out, grads, "golden, p = 0.25")
    assert bool((grads["W_dec"][:, :2 * C, :] == 0).all())
    evl, _ = _front_gpu(c0, dev, p, False, seed)      # evaluation mode: no dropout, bit for bit
    assert all(torch.equal(evl[k], plain[k]) for k in plain)


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------
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
    """the device kernels of one eager forward + backward, by name (the profiler does not trace the kernels of a replayed hipGraph)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        _run(m, static)
    return [e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset"))]


def test_forward_backward_under_graph_capture():
    """forward + backward of the small model captured on one stream: with sample_override two replays give the eager run's numbers, on
    either path, and the step with the fused stages holds fewer kernels than the composed one"""
    dev = _dev()
    from immtsf import config
    counts = {}
    for fused in (True, False):
        config.informer_model_fused = fused
        try:
            m, batch, (z, _, _, samples) = _golden_model("model_informer", dev)
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
            names = _kernels_of_a_step(m, static)
            counts[fused] = len(names)
            assert (sum("informer_" in n for n in names) == 6) == fused, names
            del graph
        finally:
            config.informer_model_fused = True
    print(f"kernels per forward + backward: fused stages {counts[True]}, composed {counts[False]}")
    assert 0 < counts[True] < counts[False]
