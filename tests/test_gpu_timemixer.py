"""GPU parity of the TimeMixer backbone (models/TimeMixer.py::forecasting): the fused path (csrc/timemixer.hip) and the composed path
against the real reference's goldens and against the float64 restatement (tests/timemixer_ref.py, pinned to those goldens in
tests/test_timemixer_ref.py) over the smallest shapes that reach each branch of the kernels (tests/timemixer_cases.py); the in-kernel
dropout against exported masks, determinism, the fall-backs to the composed path, the knob, hipGraph capture and the evaluation engine.
Tolerances: the project's fp32 bars -- 1e-4 outputs / 3e-4 gradients relative to max, the gradient floor at 1e-2 of the largest gradient;
tests/test_timemixer_ref.py holds torch's own fp32 CPU run of the restatement 4x inside them on every shape used here."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timemixer_cases as TC  # noqa: E402
import timemixer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"model_timemixer": (3, 8, 6, 8, 12, 2, 5), "model_timemixer_odd": (3, 33, 7, 16, 32, 2, 25)}
DEFAULT = TC.CASES["e_i_defaults_no_padding"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _knob:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from immtsf import config
        self.was = config.timemixer_fused
        config.timemixer_fused = self.on

    def __exit__(self, *a):
        from immtsf import config
        config.timemixer_fused = self.was


def _run(m, batch):
    tpp, data, tp, mask, up = batch
    m.zero_grad(set_to_none=True)
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check(out, grads, want_out, want):
    e = TC.rel(out, want_out)
    diff, errs = TC.grad_errors(grads, want)
    worst = max(errs, key=errs.get)
    print(f"out {e:.2e}  worst gradient {worst} {errs[worst]:.2e}")
    assert not diff, diff
    assert e < TC.OUT_TOL
    assert not {k: v for k, v in errs.items() if not v <= TC.GRAD_TOL}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_reference_golden(name, fused):
    """both goldens of the real reference through TimeMixer(cfg).forecasting: output, every gradient, and the set without one"""
    dev = _dev()
    from models.TimeMixer import TimeMixer
    C, S, P, d, dff, E, k = FIXTURES[name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = TimeMixer(TC.config(C, S, P, d, dff, E, k, batch_size=4, device=str(dev))).train()
    sd = {key[2:]: torch.from_numpy(z[key]) for key in z.files if key.startswith("p.")}
    sd["enc_embedding.position_embedding.pe"] = m.state_dict()["enc_embedding.position_embedding.pe"]      # the fixture keeps S rows of it
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    batch = tuple(torch.from_numpy(z[key]).to(dev) for key in ("tpp", "data", "tp", "mask", "upstream"))
    with _knob(fused):
        out, grads = _run(m, batch)
    assert m.fused_calls == (1 if fused else 0)
    none = set(str(z["none"]).split("\n"))
    want = {key: (None if key in none else torch.from_numpy(z["g." + key])) for key in grads}
    _check(out, grads, torch.from_numpy(z["out"]), want)


@pytest.fixture(scope="module")
def references():
    cache = {}

    def get(name):
        if name not in cache:
            case = TC.CASES[name]
            cache[name] = TC.reference(TC.make_model("cpu", case), case, TC.make_batch("cpu", case))
        return cache[name]
    return get


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_float64_restatement(name, fused, references):
    dev = _dev()
    case = TC.CASES[name]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    with _knob(fused):
        out, grads = _run(m, batch)
    assert m.fused_calls == (1 if fused else 0)
    assert tuple(out.shape) == (case[0], case[5], case[1])
    _check(out, grads, *references(name))


def _keep_masks(dev, case, m):
    """the keep multipliers of the latest fused call, per scale (B, T_i, d): element ((off_i B + b T_i + t) d + f) of the site"""
    from immtsf import config, ops
    B, C, S, P, L, Lp, d, dff, E, k = case
    p, seed, site, cnt = m._last_drop
    T = R.scale_lengths(S, 3)
    flat = ops.dropout_keep_mask(seed, site, B * sum(T) * d, p, dev).float().cpu() / (1.0 - p)
    keep, o = [], 0
    for t in T:
        keep.append(flat[o:o + B * t * d].view(B, t, d))
        o += B * t * d
    return keep


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_in_the_kernel_matches_exported_masks(p):
    dev = _dev()
    from immtsf import config
    config.disable_device_counters()
    case = TC.CASES["j_padding"]
    m, batch = TC.make_model(dev, case, dropout=p), TC.make_batch(dev, case)
    out, grads = _run(m, batch)
    assert m.fused_calls == 1
    keep = _keep_masks(dev, case, m)
    frac = float(torch.cat([k_.flatten() for k_ in keep]).eq(0).float().mean())
    assert abs(frac - p) < 0.05
    _check(out, grads, *TC.reference(m, case, batch, keep=keep))
    out2, _ = _run(m, batch)                       # a second call draws another mask
    assert m.fused_calls == 2 and not torch.equal(out, out2)
    m.eval()                                       # eval mode applies none
    with torch.no_grad():
        oe = m.forecasting(*batch[:4])
    want, _ = TC.reference(m, case, batch)
    assert TC.rel(oe, want) < TC.OUT_TOL
    m.train()


def test_backward_is_bit_reproducible():
    dev = _dev()
    case = TC.CASES["m_300_windows"]
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    out1, g1 = _run(m, batch)
    out2, g2 = _run(m, batch)
    assert m.fused_calls == 2 and torch.equal(out1, out2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k


FALLBACKS = {
    "dft_decomp": (DEFAULT, dict(decomp_method="dft_decomp", top_k=2)),      # the coarsest scale (3 rows) has two frequency bins
    "channel_dependence": (DEFAULT, dict(channel_independence=0)),
    "max_pooling": (DEFAULT, dict(down_sampling_method="max")),
    "window_3": ((4, 5, 27, 24, 27, 24, 16, 32, 2, 25), dict(down_sampling_window=3)),
    "input_len_65": ((4, 5, 65, 24, 65, 24, 16, 32, 2, 25), {}),
    "knob_off": (DEFAULT, {}),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallback_runs_the_composed_path(name):
    """outside the fused path's options and limits: the counter stands and the forecast is the knob-off run's, bit for bit"""
    dev = _dev()
    case, over = FALLBACKS[name]
    m, batch = TC.make_model(dev, case, **over), TC.make_batch(dev, case)
    with _knob(name != "knob_off"):
        out_on, g_on = _run(m, batch)
    with _knob(False):
        out_off, g_off = _run(m, batch)
    assert m.fused_calls == 0
    assert torch.equal(out_on, out_off)
    assert {k for k, g in g_on.items() if g is None} == {k for k, g in g_off.items() if g is None}


def test_even_window_raises_the_composed_paths_error():
    dev = _dev()
    case = DEFAULT[:9] + (4,)
    m, batch = TC.make_model(dev, case), TC.make_batch(dev, case)
    kinds = []
    for knob in (True, False):
        with _knob(knob), pytest.raises(Exception) as ei:
            m.forecasting(*batch[:4])
        kinds.append(type(ei.value))
    assert kinds[0] is kinds[1] and m.fused_calls == 0


def test_data_gradient_runs_the_composed_path():
    dev = _dev()
    m = TC.make_model(dev, DEFAULT)
    tpp, data, tp, mask, up = TC.make_batch(dev, DEFAULT)
    data = data.clone().requires_grad_(True)
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    assert m.fused_calls == 0
    assert data.grad is not None and float(data.grad.abs().max()) > 0
    with _knob(False):
        out_off = m.forecasting(tpp, data, tp, mask)
    assert torch.equal(out.detach(), out_off.detach())


@pytest.mark.parametrize("what", ["bfloat16_module", "non_contiguous_parameter"])
def test_a_module_the_kernel_cannot_read_runs_the_composed_path(what):
    """parameters that are not contiguous fp32 tensors on the data's device: the composed path, silently"""
    dev = _dev()
    m = TC.make_model(dev, DEFAULT)
    tpp, data, tp, mask, _ = TC.make_batch(dev, DEFAULT)
    if what == "bfloat16_module":
        m = m.bfloat16()
        data, tp, mask = data.float(), tp.float(), mask.float()
        assert not m._fused_ok(tpp, data, tp, mask)       # (what the composed path makes of mixed dtypes is torch's business)
        return
    w = m.projection.weight
    m.projection.weight = torch.nn.Parameter(w.detach().t().contiguous().t())      # same values, column-major
    assert not m.projection.weight.is_contiguous()
    with torch.no_grad():
        out_on = m.forecasting(tpp, data, tp, mask)
        with _knob(False):
            out_off = m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 0 and torch.equal(out_on, out_off)


def test_more_windows_than_the_padding_buffer_raises():
    dev = _dev()
    m = TC.make_model(dev, DEFAULT)      # batch_size 4
    case6 = (6,) + TC.CASES["j_padding"][1:]
    with pytest.raises(RuntimeError):
        m.forecasting(*TC.make_batch(dev, case6)[:4])
    assert m.fused_calls == 0
    full = (6,) + DEFAULT[1:]            # a full history needs no padding: the reference takes it
    assert m.forecasting(*TC.make_batch(dev, full)[:4]).shape == (6, 24, 5)
    assert m.fused_calls == 1


def test_knob_fused_vs_composed():
    dev = _dev()
    from immtsf import config
    m, batch = TC.make_model(dev, DEFAULT), TC.make_batch(dev, DEFAULT)
    with _knob(True):
        out_f, g_f = _run(m, batch)
    with _knob(False):
        out_c, g_c = _run(m, batch)
    assert m.fused_calls == 1
    assert TC.rel(out_f, out_c) < 1e-5
    diff, errs = TC.grad_errors(g_f, g_c)
    assert not diff and max(errs.values()) <= TC.GRAD_TOL
    try:      # the fused path is fp32 in bf16 mode too
        config.precision = "bf16"
        with _knob(True):
            out_b, _ = _run(m, batch)
    finally:
        config.precision = "fp32"
    assert torch.equal(out_b, out_f)


def _capture(m, static):
    dev = static[0].device
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(m, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.forecasting(static[0], static[1], static[2], static[3])
        (out * static[4]).sum().backward()
    return graph, out


def test_forward_backward_under_graph_capture():
    """forward + backward captured once, replayed three times on a second batch: the numbers of an eager run on that batch, bit for bit"""
    dev = _dev()
    m = TC.make_model(dev, DEFAULT)
    first, second = TC.make_batch(dev, DEFAULT, seed=7), TC.make_batch(dev, DEFAULT, seed=8)
    want_out, want_g = _run(copy.deepcopy(m), second)
    static = tuple(t.clone() for t in first)
    graph, out = _capture(m, static)
    for s, t in zip(static, second):
        s.copy_(t)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.detach(), want_out)
        for k, p in m.named_parameters():
            assert (p.grad is None and want_g[k] is None) or torch.equal(p.grad, want_g[k]), k


def test_captured_graph_holds_one_forward_and_two_backward_kernels():
    """the launch count is the acceptance figure: the kernels of ONE replay of the captured forward + backward, by name"""
    dev = _dev()
    m = TC.make_model(dev, DEFAULT)
    static = tuple(t.clone() for t in TC.make_batch(dev, DEFAULT))
    graph, _ = _capture(m, static)
    graph.replay()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        graph.replay()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "timemixer" in e.name and "kernel" in e.name]
    print(names)
    assert sum("timemixer_fwd_kernel" in n for n in names) == 1
    assert 1 <= sum("timemixer_bwd_kernel" in n or "timemixer_fold_kernel" in n for n in names) <= 2


def test_replays_under_dropout_draw_fresh_masks():
    dev = _dev()
    from immtsf import config
    m = TC.make_model(dev, DEFAULT, dropout=0.5)
    config.enable_device_counters(dev)
    try:
        _, step = config.enable_device_counters(dev)
        static = tuple(t.clone() for t in TC.make_batch(dev, DEFAULT))
        graph, out = _capture(m, static)
        outs = []
        for _ in range(3):
            step.add_(1)
            graph.replay()
            torch.cuda.synchronize()
            outs.append(out.detach().clone())
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    finally:
        config.disable_device_counters()


def test_evalstep_serves_a_timemixer_and_keys_the_knob():
    dev = _dev()
    import immtsf
    m = TC.make_model(dev, DEFAULT).eval()
    batches = []
    for seed in (11, 12):
        tpp, data, tp, mask, truth = TC.make_batch(dev, DEFAULT, seed=seed)
        batches.append({"tp_to_predict": tpp, "observed_data": data, "observed_tp": tp, "observed_mask": mask, "data_to_predict": truth,
                        "mask_predicted_data": (truth > -0.5).float()})
    ev = immtsf.EvalStep(m, None)
    n0 = m.fused_calls
    for b in batches:
        ev(b)
    assert (ev.eager, ev.captures, ev.replays) == (1, 1, 1)
    assert m.fused_calls > n0
    got = ev.result()
    nog = immtsf.EvalStep(m, None, graph=False)
    for b in batches:
        nog(b)
    ref = nog.result()
    for key in ref:
        assert got[key] == pytest.approx(ref[key], rel=1e-12), key
    with _knob(True):
        k_on = ev._key(batches[0], sorted(batches[0]))
    with _knob(False):
        k_off = ev._key(batches[0], sorted(batches[0]))
    assert k_on != k_off
