"""GPU parity of the TTM backbone (models/TTM.py, layers/MLP.py, csrc/ttm.hip): both paths against the real reference's goldens; the
narrow mixer kernel and the gate kernel against the float64 restatement (tests/ttm_ref.py, pinned to those goldens in
tests/test_ttm_ref.py) at the smallest shapes that reach each branch of the kernels; the in-kernel dropout against exported masks;
determinism, the fall-backs to the composed path, hipGraph capture with the kernel count, and the evaluation engine.
Tolerances: the project's fp32 bars -- 1e-4 outputs / 3e-4 gradients relative to max, the gradient floor at 1e-2 of the largest gradient."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ttm_cases as TC  # noqa: E402
import ttm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("x",) + R.BLOCK_KEYS

# mode, (B, M, N, D): the mixed axis is N (patch) or M (channel)
BLOCKS = {
    "a_patch_one_group_one_column": ("patch", (1, 1, 2, 1)),
    "b_patch_5_8_3": ("patch", (1, 5, 8, 3)),
    "c_channel_7_by_65": ("channel", (2, 7, 3, 65)),                 # two chunks of three groups; 65 columns: no multiple of 4
    "d_channel_17_by_1024": ("channel", (1, 17, 1, 1024)),           # the defaults' block: rows across several waves, eight column passes
    "e_patch_limit_32": ("patch", (1, 3, 32, 64)),
    "f_patch_35_groups_of_3": ("patch", (5, 7, 2, 3)),               # 16 groups per chunk: the last chunk holds three
    "g_patch_2100_groups_of_257": ("patch", (1, 2100, 2, 257)),      # more chunks than workgroups in both directions; a pass of one column
}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class _knob:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from immtsf import config
        self.was = config.ttm_fused
        config.ttm_fused = self.on

    def __exit__(self, *a):
        from immtsf import config
        config.ttm_fused = self.was


def _run(m, batch):
    tpp, data, tp, mask, up = batch
    m.zero_grad(set_to_none=True)
    out = m.forecasting(tpp, data, tp, mask)
    (out * up).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def _check(out, grads, want_out, want, out_tol=TC.OUT_TOL, grad_tol=TC.GRAD_TOL):
    e = TC.rel(out, want_out)
    diff, errs = TC.grad_errors(grads, want)
    worst = max(errs, key=errs.get)
    print(f"out {e:.2e}  worst gradient {worst} {errs[worst]:.2e}")
    assert not diff, diff
    assert e < out_tol
    assert not {k: v for k, v in errs.items() if not v <= grad_tol}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("name", sorted(TC.FIXTURES))
def test_reference_golden(name, fused):
    """the three goldens of the real reference through TTM(cfg).forecasting: output and every gradient, on both paths"""
    dev = _dev()
    m, batch, (z, params, none) = TC.golden_model(name, dev)
    with _knob(fused):
        out, grads = _run(m, batch)
    assert m.fused_blocks == (len(m.mixer_blocks()) if fused else 0)
    want = {key: (None if key in none else torch.from_numpy(z["g." + key])) for key in grads}
    _check(out, grads, torch.from_numpy(z["out"]), want)


def _block(dev, mode, shape, p=0.0, seed=0):
    from layers.MLP import TTMMixerBlock
    B, M, N, D = shape
    x, up, params = TC.block_tensors(B, M, N, D, mode, seed=seed)
    blk = TTMMixerBlock(d_model=D, features=N if mode == "patch" else M, mode=mode, dropout=p)
    blk.load_state_dict(dict(zip(R.BLOCK_KEYS, params)))
    return blk.to(dev).train(), x.to(dev), up.to(dev), params


def _run_block(blk, x, up):
    x = x.clone().requires_grad_(True)
    blk.zero_grad(set_to_none=True)
    out = blk(x)
    (out * up).sum().backward()
    sd = dict(blk.named_parameters())
    return out.detach(), dict(zip(NAMES, [x.grad.clone()] + [sd[k].grad.clone() for k in R.BLOCK_KEYS]))


def _keep(dev, blk, mode, shape):
    """the keep multipliers of the block's latest kernel call in the kernel's element order: (G, D, 2F) and (G, D, F)"""
    from immtsf import ops
    B, M, N, D = shape
    G, Fm = (B * M, N) if mode == "patch" else (B * N, M)
    p, seed, site, cnt = blk._last_drop
    out = []
    for s, width in ((site, 2 * Fm), (site + 1, Fm)):
        stride = (width + 3) // 4 * 4      # a column's draws start on a Philox call
        flat = ops.dropout_keep_mask(seed, s, G * D * stride, p, dev).float().cpu() / (1.0 - p)
        out.append(flat.view(G, D, stride)[:, :, :width])
    return tuple(out)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_narrow_kernel_matches_float64_block(name, p):
    """forward, dx and the eight parameter gradients of one launch forward / two backward against the restatement of one block"""
    dev = _dev()
    from immtsf import config
    config.disable_device_counters()
    mode, shape = BLOCKS[name]
    blk, x, up, params = _block(dev, mode, shape, p=p)
    out, grads = _run_block(blk, x, up)
    assert blk.took_kernel
    keep = _keep(dev, blk, mode, shape) if p > 0 else None
    want_out, want_dx, want_g = R.run_block(x, params, up, mode, keep=keep)
    _check(out, grads, want_out, dict(zip(NAMES, [want_dx] + want_g)))


def test_narrow_kernel_dropout_matches_exported_masks():
    dev = _dev()
    from immtsf import config
    config.disable_device_counters()
    mode, shape = BLOCKS["c_channel_7_by_65"]
    blk, x, up, params = _block(dev, mode, shape, p=0.5)
    out, grads = _run_block(blk, x, up)
    keep = _keep(dev, blk, mode, shape)
    for k in keep:
        assert abs(float(k.eq(0).float().mean()) - 0.5) < 0.05
    want_out, want_dx, want_g = R.run_block(x, params, up, mode, keep=keep)
    _check(out, grads, want_out, dict(zip(NAMES, [want_dx] + want_g)))
    out2, _ = _run_block(blk, x, up)               # a second call draws another mask
    assert not torch.equal(out, out2)
    blk.eval()                                     # eval mode applies none
    with torch.no_grad():
        oe = blk(x)
    assert blk.took_kernel and TC.rel(oe, R.run_block(x, params, up, mode)[0]) < TC.OUT_TOL


def _capture_block(blk, x, up):
    from immtsf import step_plan
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream(device=x.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (blk(xs) * up).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    blk.zero_grad(set_to_none=True)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    step_plan.collect_before_capture()
    with torch.cuda.graph(graph):
        out = blk(xs)
        (out * up).sum().backward()
    return graph, out, xs


def test_replays_under_dropout_draw_fresh_masks():
    dev = _dev()
    from immtsf import config
    mode, shape = BLOCKS["c_channel_7_by_65"]
    blk, x, up, _ = _block(dev, mode, shape, p=0.5)
    try:
        _, step = config.enable_device_counters(dev)
        graph, out, _ = _capture_block(blk, x, up)
        outs = []
        for _ in range(3):
            step.add_(1)
            graph.replay()
            torch.cuda.synchronize()
            outs.append(out.detach().clone())
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])
    finally:
        config.disable_device_counters()


def test_captured_block_holds_one_forward_and_at_most_three_backward_kernels():
    """the launch count is the acceptance figure: the kernels of ONE replay of a captured narrow block, by name"""
    dev = _dev()
    mode, shape = BLOCKS["c_channel_7_by_65"]
    blk, x, up, _ = _block(dev, mode, shape)
    graph, _, _ = _capture_block(blk, x, up)
    graph.replay()
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        graph.replay()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if "ttm_" in e.name and "kernel" in e.name]
    print(names)
    assert sum("ttm_mixer_fwd_kernel" in n for n in names) == 1
    assert 1 <= sum("ttm_mixer_bwd_kernel" in n or "ttm_mixer_fold_kernel" in n for n in names) <= 3


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("d", [1, 3, 64, 1000, 4096])
def test_gate_kernel_matches_float64(d, rows):
    dev = _dev()
    from immtsf import ops
    g_ = torch.Generator().manual_seed(d * 100 + rows)
    res, u, g, up = (torch.randn(rows, d, generator=g_) for _ in range(4))
    g[rows // 2, d // 3] += 80.0                   # one logit far above the rest: the softmax must not overflow
    t = [v.to(dev).requires_grad_(True) for v in (res, u, g)]
    out = ops.ttm_gate(*t)
    (out * up.to(dev)).sum().backward()
    w = [v.double().requires_grad_(True) for v in (res, u, g)]
    want = R.gate(*w)
    (want * up.double()).sum().backward()
    assert torch.isfinite(out).all()
    _check(out, {k: v.grad for k, v in zip(("res", "u", "g"), t)}, want, {k: v.grad for k, v in zip(("res", "u", "g"), w)})


def test_backward_is_bit_reproducible():
    dev = _dev()
    mode, shape = BLOCKS["g_patch_2100_groups_of_257"]
    blk, x, up, _ = _block(dev, mode, shape, seed=3)
    out1, g1 = _run_block(blk, x, up)
    out2, g2 = _run_block(blk, x, up)
    assert torch.equal(out1, out2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    m, batch, _ = TC.golden_model("model_ttm_odd", dev)      # ... and the narrow blocks' gradients of a whole model
    _, a = _run(m, batch)
    _, b = _run(m, batch)
    for k in a:
        if ".patch_mixer." in k or ".channel_feature_mixer." in k:
            assert torch.equal(a[k], b[k]), k


def test_mixed_axis_of_33_runs_the_composed_path():
    dev = _dev()
    blk, x, up, _ = _block(dev, "channel", (2, 33, 2, 8))
    with _knob(True):
        out_on, g_on = _run_block(blk, x, up)
        assert not blk.took_kernel
    with _knob(False):
        out_off, g_off = _run_block(blk, x, up)
    assert torch.equal(out_on, out_off)
    # the composed backward is the same code under either knob, but its small GEMMs add the weight gradients with float atomics, whose
    # order is free: equal up to that reordering (64 terms of fp32 rounding, 6e-8 each, stay below 1e-5 of the largest entry)
    diff, errs = TC.grad_errors(g_on, g_off)
    assert not diff and max(errs.values()) < 1e-5, errs
    blk32, x32, up32, _ = _block(dev, "channel", (2, 32, 2, 8))
    _run_block(blk32, x32, up32)
    assert blk32.took_kernel


@pytest.mark.parametrize("what", ["bfloat16_module", "non_contiguous_parameter"])
def test_a_block_the_kernel_cannot_read_runs_the_composed_path(what):
    dev = _dev()
    blk, x, up, _ = _block(dev, "patch", (2, 3, 4, 8))
    assert blk.kernel_ok(x)
    if what == "bfloat16_module":      # the composed path widens the parameters and computes in fp32: the restatement on the rounded values
        blk = blk.bfloat16()
        assert not blk.kernel_ok(x)
        out, grads = _run_block(blk, x, up)
        assert not blk.took_kernel and out.dtype == torch.float32
        sd = blk.state_dict()
        assert all(sd[k].dtype == torch.bfloat16 for k in R.BLOCK_KEYS)
        want_out, want_dx, _ = R.run_block(x, [sd[k].float() for k in R.BLOCK_KEYS], up, "patch")
        assert TC.rel(out, want_out) < TC.OUT_TOL and TC.rel(grads["x"], want_dx) < TC.GRAD_TOL
        return
    w = blk.mlp.fc1.weight
    blk.mlp.fc1.weight = torch.nn.Parameter(w.detach().t().contiguous().t())      # same values, column-major
    assert not blk.mlp.fc1.weight.is_contiguous()
    with torch.no_grad():
        out_on = blk(x)
        assert not blk.took_kernel
        with _knob(False):
            out_off = blk(x)
    assert torch.equal(out_on, out_off)


def test_more_windows_than_the_padding_buffer_raises_and_a_wrong_channel_count_asserts():
    dev = _dev()
    m, (tpp, data, tp, mask, up), _ = TC.golden_model("model_ttm", dev)      # batch_size 4, L = 6 < input_len 8
    six = [torch.cat([t, t], 0) for t in (tpp, data, tp, mask)]
    with pytest.raises(RuntimeError):
        m.forecasting(*six)
    with pytest.raises(AssertionError):
        m.forecasting(tpp, data[:, :, :2], tp, mask[:, :, :2])
    g = torch.Generator().manual_seed(5)
    full = torch.randn(6, 8, 3, generator=g).to(dev)      # a full history needs no padding: the reference takes it
    out = m.forecasting(six[0], full, torch.sort(torch.rand(6, 8, generator=g), 1).values.to(dev), torch.ones(6, 8, 3, device=dev))
    assert out.shape == (6, 4, 3) and m.fused_blocks == len(m.mixer_blocks())


def test_data_gradient_and_knob():
    """a data tensor that wants a gradient still takes the kernels (dx exists); knob on and off agree; the kernels are fp32 in bf16 mode"""
    dev = _dev()
    from immtsf import config
    m, (tpp, data, tp, mask, up), _ = TC.golden_model("model_ttm", dev)
    d1 = data.clone().requires_grad_(True)
    (m.forecasting(tpp, d1, tp, mask) * up).sum().backward()
    assert m.fused_blocks == len(m.mixer_blocks())
    with _knob(False):
        d0 = data.clone().requires_grad_(True)
        (m.forecasting(tpp, d0, tp, mask) * up).sum().backward()
    assert m.fused_blocks == 0 and float(d0.grad.abs().max()) > 0
    assert TC.rel(d1.grad, d0.grad) < TC.GRAD_TOL
    out_f, g_f = _run(m, (tpp, data, tp, mask, up))
    with _knob(False):
        out_c, g_c = _run(m, (tpp, data, tp, mask, up))
    assert TC.rel(out_f, out_c) < 1e-5
    diff, errs = TC.grad_errors(g_f, g_c)
    assert not diff and max(errs.values()) <= TC.GRAD_TOL
    blk, x, xup, _ = _block(dev, "channel", (2, 7, 3, 65))
    ob_f, gb_f = _run_block(blk, x, xup)
    try:      # bf16 mode changes the GEMMs behind linear() and nothing in the kernels
        config.precision = "bf16"
        _run(m, (tpp, data, tp, mask, up))
        assert m.fused_blocks == len(m.mixer_blocks())
        ob_b, gb_b = _run_block(blk, x, xup)
    finally:
        config.precision = "fp32"
    assert torch.equal(ob_b, ob_f) and all(torch.equal(gb_b[k], gb_f[k]) for k in gb_f)


def test_forward_backward_under_graph_capture():
    """forward + backward of model_ttm captured once and replayed three times: the eager run's numbers (the GEMMs' weight gradients are
    split-K sums, so to 1e-5 rather than bit for bit)"""
    dev = _dev()
    from immtsf import step_plan
    m, batch, _ = TC.golden_model("model_ttm", dev)
    want_out, want_g = _run(copy.deepcopy(m), batch)
    static = tuple(t.clone() for t in batch)
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
        out = m.forecasting(static[0], static[1], static[2], static[3])
        (out * static[4]).sum().backward()
    assert m.fused_blocks == len(m.mixer_blocks())
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        _check(out, {k: p.grad for k, p in m.named_parameters()}, want_out, want_g, out_tol=1e-5, grad_tol=1e-5)


def test_evalstep_serves_a_ttm_and_keys_the_knob():
    dev = _dev()
    import immtsf
    m, (tpp, data, tp, mask, up), _ = TC.golden_model("model_ttm", dev)
    m.eval()
    batches = []
    for seed in (11, 12):
        g = torch.Generator().manual_seed(seed)
        truth = torch.randn(3, 4, 3, generator=g).to(dev)
        batches.append({"tp_to_predict": tpp, "observed_data": data + 0.01 * seed, "observed_tp": tp, "observed_mask": mask,
                        "data_to_predict": truth, "mask_predicted_data": (truth > -0.5).float()})
    ev = immtsf.EvalStep(m, None)
    for b in batches:
        ev(b)
    assert (ev.eager, ev.captures, ev.replays) == (1, 1, 1)
    assert m.fused_blocks == len(m.mixer_blocks())
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
