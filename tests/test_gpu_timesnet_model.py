"""models.TimesNet's fused front end and output tail (csrc/timesnet_model.hip, the row-offset tail of csrc/informer.hip) on the GPU: each
stage against its float64 restatement (tests/timesnet_model_ref.py, pinned in tests/test_timesnet_model_ref.py) on every case of
tests/timesnet_model_cases.py, forecasting() with the knob on against the knob off and against the golden of the unmodified reference,
which route runs, the dropout mask of both routes, bit-identical reruns, graph capture with the kernel counts, and the ABI's refusals.
Bars: the project's fp32 bars as tests/test_gpu_informer_model.py uses them (1e-4 outputs, 3e-4 gradients, relative to the tensor's
largest magnitude)."""
import os
import sys

import pytest
import torch

import timesnet_model_cases as TC

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


# ---- 1. the front stage against float64 --------------------------------------------------------------------------------------------------
def _front_gpu(name, dev, p=0.0, training=False, seed=None, save_e=None):
    from immtsf import ops
    B, L, S, Lp, P, C, D = TC.CASES[name]
    t = {k: v.to(dev) for k, v in TC.inputs(name).items()}
    for k in ("W_token", "W_predict", "b_predict"):
        t[k].requires_grad_(True)
    enc, means, stdev = ops.timesnet_front(t["data"], t["mask"], t["tp"], t["tpp"], S, P, t["W_token"], t["pe"], t["W_predict"], t["b_predict"],
                                           p, training, seed, save_e)
    (enc * t["up_enc"]).sum().backward()
    torch.cuda.synchronize()
    return dict(enc=enc.detach(), means=means, stdev=stdev), {k: t[k].grad for k in ("W_token", "W_predict", "b_predict")}


def _front_check(ref, out, grads, label):
    errs_o = {k: TC.rel(out[k], w) for k, w in ref["want"].items()}
    diff, errs = TC.grad_errors(grads, ref["grads"])
    for k, v in {**errs_o, **errs}.items():
        print(f"MEASURED | timesnet_front {label} | {k} | {v:.3g} | bar {TC.OUT_TOL if k in errs_o else TC.GRAD_TOL:.3g}")
    assert max(errs_o.values()) < TC.OUT_TOL and not diff and max(errs.values()) < TC.GRAD_TOL, (errs_o, errs)


@pytest.mark.parametrize("save_e", [False, True])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_front_matches_float64(name, save_e):
    dev = _dev()
    from immtsf import ops
    B, L, S, Lp, P, C, D = TC.CASES[name]
    assert ops.timesnet_model_supported(S, P, C, D)
    out, grads = _front_gpu(name, dev, save_e=save_e)
    assert tuple(out["enc"].shape) == (B, S + P, D) and tuple(out["means"].shape) == (B, 1, C) and tuple(out["stdev"].shape) == (B, 1, C)
    _front_check(TC.front_reference(name), out, grads, f"{name}{' (E saved)' if save_e else ''}")
    out2, grads2 = _front_gpu(name, dev, save_e=save_e)      # two runs: the same bits
    assert all(torch.equal(out[k], out2[k]) for k in out) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    if name == "flat":
        floor = 1e-5 ** 0.5
        assert float(out["means"][0, 0, 1]) == 2.5 and abs(float(out["stdev"][0, 0, 1]) - floor) < 1e-6 * floor


def test_front_statistics_are_the_composed_routes_bits():
    """means / stdev are immtsf_instance_norm's sums in the same order: equal bits, so the de-normalisation is the same on either route"""
    dev = _dev()
    from models._common import pad_history, plain_instance_norm
    B, L, S, Lp, P, C, D = TC.CASES["ragged"]
    t = {k: v.to(dev) for k, v in TC.inputs("ragged").items()}
    zeros = torch.zeros(B, max(S, P), C, device=dev)
    _, data, _, _, _ = pad_history(zeros, S, P, t["tpp"], t["data"], t["tp"], t["mask"])
    _, means, stdev = plain_instance_norm(data)
    out, _ = _front_gpu("ragged", dev)
    assert torch.equal(out["means"], means) and torch.equal(out["stdev"], stdev)


# ---- 2. the tail stage against float64 ---------------------------------------------------------------------------------------------------
def _tail_gpu(name, dev):
    from immtsf import ops
    B, L, S, Lp, P, C, D = TC.CASES[name]
    t = TC.inputs(name)
    norm, proj = torch.nn.LayerNorm(D), torch.nn.Linear(D, C)
    with torch.no_grad():
        norm.weight.copy_(t["gamma"]), norm.bias.copy_(t["beta"])
        proj.weight.copy_(t["W"]), proj.bias.copy_(t["b"])
    norm, proj = norm.to(dev), proj.to(dev)
    x = t["x"].to(dev).requires_grad_(True)
    y = ops.timesnet_tail(x, norm, proj, t["means"].to(dev), t["stdev"].to(dev), S, Lp)
    (y * t["up_y"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), dict(x=x.grad, gamma=norm.weight.grad, beta=norm.bias.grad, W=proj.weight.grad, b=proj.bias.grad)


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_tail_matches_float64(name):
    dev = _dev()
    B, L, S, Lp, P, C, D = TC.CASES[name]
    ref = TC.tail_reference(name)
    y, grads = _tail_gpu(name, dev)
    assert y.is_contiguous() and tuple(y.shape) == (B, Lp, C)
    eo = TC.rel(y, ref["out"])
    diff, errs = TC.grad_errors(grads, ref["grads"])
    for k, v in {"y": eo, **errs}.items():
        print(f"MEASURED | timesnet_tail {name} | {k} | {v:.3g} | bar {TC.OUT_TOL if k == 'y' else TC.GRAD_TOL:.3g}")
    assert eo < TC.OUT_TOL and not diff and max(errs.values()) < TC.GRAD_TOL, errs
    gx = grads["x"]
    assert tuple(gx.shape) == (B, S + P, D) and bool((gx[:, :S] == 0).all()) and bool((gx[:, S + Lp:] == 0).all()), \
        "dx outside the horizon rows must be exact zeros"
    y2, grads2 = _tail_gpu(name, dev)      # two runs: the same bits
    assert torch.equal(y, y2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- 3. forecasting(): the knob on against the knob off, and the golden ---------------------------------------------------------------------
def _golden_model(dev, **over):
    from models.TimesNet import TimesNet
    z, params = TC.golden()
    m = TimesNet(TC.config(dev, **over))
    m.load_state_dict(params, strict=True)
    m = m.to(dev).train()
    batch = tuple(torch.from_numpy(z[k]).to(dev) for k in ("tpp", "data", "tp", "mask", "upstream"))
    return m, batch, z


def _run(m, batch):
    m.zero_grad(set_to_none=True)
    out = m.forecasting(*batch[:4])
    (out * batch[4]).sum().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}


def test_forecasting_knob_on_against_knob_off_and_the_golden(monkeypatch):
    dev = _dev()
    from immtsf import config
    m, batch, z = _golden_model(dev)
    monkeypatch.setattr(config, "timesnet_model_fused", True)
    out_on, g_on = _run(m, batch)
    assert m.fused_calls == 1
    monkeypatch.setattr(config, "timesnet_model_fused", False)
    out_off, g_off = _run(m, batch)
    assert m.fused_calls == 1
    want = {k: torch.from_numpy(z["g." + k]) for k, _ in m.named_parameters()}
    for label, out, grads, ref_out, ref_g in (("on vs off", out_on, g_on, out_off, g_off), ("on vs golden", out_on, g_on, z["out"], want),
                                              ("off vs golden", out_off, g_off, z["out"], want)):
        eo = TC.rel(out, ref_out)
        grads = {k: (torch.zeros_like(dict(m.named_parameters())[k]) if v is None else v) for k, v in grads.items()}
        ref_g = {k: (torch.zeros_like(grads[k]) if v is None else v) for k, v in ref_g.items()}
        diff, errs = TC.grad_errors(grads, ref_g)
        print(f"MEASURED | forecasting {label} | out {eo:.3g} | worst gradient {max(errs.values()):.3g} ({max(errs, key=errs.get)})")
        assert out.shape == tuple(z["out"].shape) and eo < TC.OUT_TOL and not diff and max(errs.values()) < TC.GRAD_TOL, (label, errs)
    assert {k for k, v in g_on.items() if v is None} == {k for k, v in g_off.items() if v is None}


# ---- 4. which route runs ----------------------------------------------------------------------------------------------------------------------
def test_routes(monkeypatch):
    dev = _dev()
    from immtsf import config
    monkeypatch.setattr(config, "timesnet_model_fused", True)
    m, batch, z = _golden_model(dev)
    tpp, data, tp, mask, up = batch
    want = torch.from_numpy(z["out"])
    out = m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 1 and TC.rel(out, want) < TC.OUT_TOL
    monkeypatch.setattr(config, "timesnet_model_fused", False)                      # IMMTSF_TIMESNET_MODEL_FUSED=0
    out = m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 1 and TC.rel(out, want) < TC.OUT_TOL
    monkeypatch.setattr(config, "timesnet_model_fused", True)
    d2 = data.clone().requires_grad_(True)                                          # an input that wants a gradient
    out = m.forecasting(tpp, d2, tp, mask)
    out.sum().backward()
    assert m.fused_calls == 1 and d2.grad is not None and TC.rel(out, want) < TC.OUT_TOL
    long = m.input_len + 1                                                          # L > input_len: the composed path's own behaviour
    g = torch.Generator().manual_seed(5)
    # (the routing decision alone: behind it the composed path hands predict_linear a series longer than its weight, and immtsf.ops.linear
    # does not compare the two -- nothing a test should launch)
    assert not m._fused_ok(tpp, torch.randn(3, long, 3, generator=g).to(dev), torch.rand(3, long, generator=g).to(dev),
                           torch.ones(3, long, 3, device=dev))
    assert m._fused_ok(tpp, data, tp, mask) and m.fused_calls == 1
    md, _, _ = _golden_model(dev)
    md = md.double()                                                                # a .double() model: whatever the composed path does
    try:
        md.forecasting(tpp.double(), data.double(), tp.double(), mask.double())
    except Exception as e:
        print(f"composed path with a .double() model: {type(e).__name__}: {e}")
    assert md.fused_calls == 0
    out = m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 2


def test_more_windows_than_the_padding_buffer_fails_as_the_reference_does():
    dev = _dev()
    m, (tpp, data, tp, mask, up), _ = _golden_model(dev, batch_size=2)
    with pytest.raises(RuntimeError):
        m.forecasting(tpp, data, tp, mask)                                          # 3 windows to pad from 2 rows of zeros
    assert m.fused_calls == 0


def test_c_out_other_than_enc_in_reaches_the_composed_paths_error():
    dev = _dev()
    from models.TimesNet import TimesNet
    _, (tpp, data, tp, mask, up), _ = _golden_model(dev)
    torch.manual_seed(0)
    m = TimesNet(TC.config(dev, c_out=2)).to(dev).train()
    with pytest.raises(RuntimeError):
        m.forecasting(tpp, data, tp, mask)
    assert m.fused_calls == 0


# ---- 5. dropout ---------------------------------------------------------------------------------------------------------------------------------
def test_both_routes_draw_the_same_dropout_mask(monkeypatch):
    """dropout 0.1 in training mode, the seed counter at the same value before each call: one seed consumed on either route, the same
    Philox site and element index, so the same elements of the embedding are zero and the forecasts agree to fp32 rounding"""
    dev = _dev()
    from immtsf import config
    m, batch, z = _golden_model(dev, dropout=0.1)
    assert m.enc_embedding.dropout.p == 0.1
    res = {}
    for on in (True, False):
        monkeypatch.setattr(config, "timesnet_model_fused", on)
        monkeypatch.setattr(config, "_counter", 41)
        res[on] = _run(m, batch)
        assert config._counter == 42, "one next_seed() per call on either route"
    assert m.fused_calls == 1
    eo = TC.rel(res[True][0], res[False][0])
    diff, errs = TC.grad_errors({k: v for k, v in res[True][1].items() if v is not None}, {k: v for k, v in res[False][1].items() if v is not None})
    print(f"MEASURED | forecasting with dropout 0.1, on vs off | out {eo:.3g} | worst gradient {max(errs.values()):.3g}")
    assert eo < TC.OUT_TOL and not diff and max(errs.values()) < TC.GRAD_TOL, errs
    monkeypatch.setattr(config, "timesnet_model_fused", True)
    monkeypatch.setattr(config, "_counter", 41)
    plain = m.eval().forecasting(*batch[:4])
    assert config._counter == 41 and TC.rel(plain, z["out"]) < TC.OUT_TOL, "no seed and no dropout in evaluation mode"


def test_front_dropout_is_token_embeds_mask(monkeypatch):
    """the stage with p 0.25 against float64 under the exported keep-mask of token_embed's site, and the fraction of exact zeros of the
    embedded rows equal on both routes"""
    dev = _dev()
    from immtsf import config, ops
    monkeypatch.setattr(config, "_device_counters", {})      # the key is the seed alone
    name, p, seed = "ragged", 0.25, 0x1234_5678_9ABC
    B, L, S, Lp, P, C, D = TC.CASES[name]
    assert ops.SITE_TIMESNET_EMBED == ops.SITE_LAYER_BASE + 41
    keep = ops.dropout_keep_mask(seed, ops.SITE_TIMESNET_EMBED, B * S * D, p, dev).view(B, S, D)
    torch.cuda.synchronize()
    assert 0.6 < float(keep.float().mean()) < 0.9
    scale = keep.float().cpu() / (1 - p)
    for save_e in (False, True):
        out, grads = _front_gpu(name, dev, p, True, seed, save_e)
        _front_check(TC.front_reference(name, scale), out, grads, f"{name}, p = {p}{' (E saved)' if save_e else ''}")
    plain, _ = _front_gpu(name, dev)
    evl, _ = _front_gpu(name, dev, p, False, seed)            # evaluation mode: no dropout, bit for bit
    assert all(torch.equal(evl[k], plain[k]) for k in plain)
    # the composed route's embedding under the same seed: token_embed draws next_seed() itself
    t = {k: v.to(dev) for k, v in TC.inputs(name).items()}
    z = torch.zeros(B, S - L, C, device=dev)
    x = torch.cat([torch.cat([t["data"], z], 1), torch.cat([t["mask"], z], 1), torch.cat([t["tp"], z[:, :, 0]], 1).unsqueeze(-1)], -1)
    monkeypatch.setattr(config, "next_seed", lambda: seed)
    emb = ops.token_embed(x, t["W_token"], t["pe"][:S], p, True)
    torch.cuda.synchronize()
    zeros_composed = (emb == 0)
    assert torch.equal(zeros_composed, keep == 0), "token_embed's zeros are the exported mask's"
    assert float(zeros_composed.float().mean()) == float((keep == 0).float().mean())


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------------
def test_bench_step_replays_from_a_graph_with_fewer_kernels():
    """tools/timesnet_bench.py --model's step (forecasting() + backward at cfg4's dimensions, 4 windows) captured with the knob on: the
    replay reproduces the eager step, and the graph holds strictly fewer kernels than the knob-off graph"""
    _dev()
    import timesnet_bench as TB
    models, step = TB.make("cfg4", B=4, model=True)
    m = models["fused"]
    m.zero_grad(set_to_none=True)
    out_e = step("fused").detach().clone()
    torch.cuda.synchronize()
    assert m.fused_calls == 1
    grads_e = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    graph, out = TB.capture(models, step, "fused")
    out.zero_()
    for p in m.parameters():
        if p.grad is not None:
            p.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and TC.rel(out, out_e) <= TC.OUT_TOL
    diff, errs = TC.grad_errors({k: p.grad for k, p in m.named_parameters() if k in grads_e}, grads_e)
    assert not diff and max(errs.values()) <= TC.GRAD_TOL, errs
    graph_off, _ = TB.capture(models, step, "torch")
    assert models["torch"].fused_calls == 0
    n_on, n_off = TB.count_kernels(graph), TB.count_kernels(graph_off)
    print(f"MEASURED | graph kernels, cfg4 dimensions, B 4 | knob on {n_on} | knob off {n_off}")
    assert 0 < n_on < n_off, (n_on, n_off)


# ---- 7. the ABI's refusals: no launch, no fault ------------------------------------------------------------------------------------------------
def test_abi_refuses_null_pointers_and_unsupported_dimensions():
    dev = _dev()
    from immtsf import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -2
    B, L, S, Lp, P, C, D = TC.CASES["ragged"]
    T = S + P
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    ok, s, none = _lib.ptr(buf), _lib.stream_ptr(), None
    front_f = lambda dims, ptrs: lib.immtsf_timesnet_front_forward(*dims, *ptrs, 0.0, 0, 57, None, s)
    front_b = lambda dims, ptrs, ws=(ok, buf.numel() * 4): lib.immtsf_timesnet_front_backward(*dims, *ptrs, 0.0, 0, 57, None, *ws, s)
    dims = (B, L, S, Lp, P, C, D)
    for i in range(11):
        assert front_f(dims, [none if j == i else ok for j in range(12)]) == EINVAL, i
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11):
        assert front_b(dims, [none if j == i else ok for j in range(12)]) == EINVAL, i
    assert front_b(dims, [ok] * 12, (none, 1 << 20)) == EINVAL and front_b(dims, [ok] * 12, (ok, 16)) == EWORKSPACE
    bad = [(B, L, S, Lp, P, C, 18), (B, L, S, Lp, P, 11, D), (B, L, 200, Lp, 57, C, D), (B, S + 1, S, Lp, P, C, D), (B, L, S, P + 1, P, C, D),
           (0, L, S, Lp, P, C, D), (B, 0, S, Lp, P, C, D)]
    for d in bad:
        assert front_f(d, [ok] * 12) == EUNSUPPORTED and front_b(d, [ok] * 12) == EUNSUPPORTED, d
        assert lib.immtsf_timesnet_model_supported(d[2], d[4], d[5], d[6]) == (0 if d in bad[:3] else 1), d
    assert lib.immtsf_timesnet_front_workspace_bytes(B, S, P, C, 18) == 0 and lib.immtsf_timesnet_front_workspace_bytes(0, S, P, C, D) == 0
    tail_f = lambda dims, ptrs: lib.immtsf_timesnet_tail_forward(*dims, *ptrs[:3], 1e-5, *ptrs[3:], s)
    tail_b = lambda dims, ptrs: lib.immtsf_timesnet_tail_backward(*dims, *ptrs, ok, buf.numel() * 4, s)
    tdims = (B, Lp, T, S, C, D)
    for i in range(10):
        assert tail_f(tdims, [none if j == i else ok for j in range(10)]) == EINVAL, i
        assert tail_b(tdims, [none if j == i else ok for j in range(10)]) == EINVAL, i
    for d in [(B, Lp, T, T - Lp + 1, C, D), (B, Lp, T, -1, C, D), (B, 0, T, S, C, D), (B, Lp, T, S, C, 18), (B, Lp, T, S, 33, D), (0, Lp, T, S, C, D)]:
        assert tail_f(d, [ok] * 10) == EUNSUPPORTED and tail_b(d, [ok] * 10) == EUNSUPPORTED, d
    torch.cuda.synchronize()
    assert bool((buf == 0).all()), "nothing was launched"


def test_sizes_beyond_the_measured_bound_take_the_composed_path(monkeypatch):
    """config.timesnet_model_max_work: the kernels take (T 192, d_model 64), the model routes it to the composed path, where it measured
    faster; without the bound the same call is fused"""
    dev = _dev()
    from immtsf import config, ops
    from models.TimesNet import TimesNet
    assert ops.timesnet_model_supported(96, 96, 8, 64) and config.timesnet_model_max_work == 64 * 64 * 16
    torch.manual_seed(0)
    m = TimesNet(TC.config(dev, input_len=96, pred_len=96, enc_in=8, c_out=8, d_model=64, d_ff=64, top_k=5, num_kernels=2)).to(dev)
    g = torch.Generator().manual_seed(2)
    batch = (torch.rand(2, 96, generator=g).to(dev), torch.randn(2, 96, 8, generator=g).to(dev), torch.rand(2, 96, generator=g).to(dev),
             torch.ones(2, 96, 8, device=dev))
    assert not m._fused_ok(*batch)
    monkeypatch.setattr(config, "timesnet_model_max_work", None)
    assert m._fused_ok(*batch)
