"""tests/timesnet_model_ref.py (the float64 yardsticks of csrc/timesnet_model.hip and of the row-offset tail) pinned on the CPU: on every
case of tests/timesnet_model_cases.py `front` is pad + instance norm + cat + conv1d(circular) + pe + cat + linear over time from
torch.nn.functional, `tail` is layer_norm + linear + de-normalisation + slice, and the written-out gradients are autograd's; around the
product's TimesBlock (the branch a CPU tensor takes) the two reproduce the golden of the unmodified reference, output and gradients."""
import pytest
import torch
import torch.nn.functional as F

import timesnet_model_cases as TC
import timesnet_model_ref as MR


def _functional_front(t, S, P, scale=None):
    data, mask, tp, tpp = t["data"], t["mask"], t["tp"], t["tpp"]
    B, L, C = data.shape
    z = data.new_zeros(B, S - L, C)
    d, m, tt = torch.cat([data, z], 1), torch.cat([mask, z], 1), torch.cat([tp, z[:, :, 0]], 1)
    tq = torch.cat([tpp, tpp.new_zeros(B, P - tpp.shape[1])], 1)
    means = d.mean(1, keepdim=True)
    x = d - means
    stdev = torch.sqrt(torch.var(x, dim=1, keepdim=True, unbiased=False) + 1e-5)
    inp = torch.cat([x / stdev, m, tt.unsqueeze(-1)], -1)
    emb = F.conv1d(F.pad(inp.permute(0, 2, 1), (1, 1), mode="circular"), t["W_token"]).transpose(1, 2) + t["pe"][:S]
    if scale is not None:
        emb = emb * scale
    enc = torch.cat([emb, tq.unsqueeze(-1).repeat(1, 1, emb.size(-1))], 1)
    enc = F.linear(enc.permute(0, 2, 1), t["W_predict"], t["b_predict"]).permute(0, 2, 1)
    return enc, means, stdev


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_front_is_torch_functional_and_its_gradients_are_autograds(name, with_scale):
    B, L, S, Lp, P, C, D = TC.CASES[name]
    t = {k: v.double() for k, v in TC.inputs(name).items()}
    scale = None
    if with_scale:
        scale = (torch.rand(B, S, D, generator=torch.Generator().manual_seed(3)) >= 0.25).double() / 0.75
    for k in ("W_token", "W_predict", "b_predict"):
        t[k].requires_grad_(True)
    want, wm, ws = _functional_front(t, S, P, scale)
    (want * t["up_enc"]).sum().backward()
    want = want.detach()
    with torch.no_grad():
        enc, means, stdev, E, inp = MR.front(t["data"], t["mask"], t["tp"], t["tpp"], S, P, t["W_token"], t["pe"], t["W_predict"],
                                             t["b_predict"], scale)
        grads = MR.front_grads(t["up_enc"], E, inp, t["W_predict"], S, scale)
    assert tuple(enc.shape) == (B, S + P, D) and tuple(means.shape) == (B, 1, C)
    for got, w in ((enc, want), (means, wm), (stdev, ws)):
        assert got.shape == w.shape and float((got - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))
    for k, gr in grads.items():
        assert gr.shape == t[k].grad.shape and float((gr - t[k].grad).abs().max()) <= 1e-12 * max(1.0, float(t[k].grad.abs().max())), k
    if name == "flat":
        floor = 1e-5 ** 0.5
        assert abs(float(stdev[0, 0, 1]) - floor) < 1e-12 and float(means[0, 0, 1]) == 2.5


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_tail_is_torch_functional_and_its_gradients_are_autograds(name):
    B, L, S, Lp, P, C, D = TC.CASES[name]
    t = {k: v.double() for k, v in TC.inputs(name).items()}
    for k in ("x", "gamma", "beta", "W", "b"):
        t[k].requires_grad_(True)
    dec = F.linear(F.layer_norm(t["x"], (D,), t["gamma"], t["beta"], 1e-5), t["W"], t["b"])
    dec = dec * t["stdev"][:, 0, :].unsqueeze(1) + t["means"][:, 0, :].unsqueeze(1)
    want = dec[:, -P:, :][:, :Lp, :]
    (want * t["up_y"]).sum().backward()
    want = want.detach()
    with torch.no_grad():
        got = MR.tail(t["x"], t["gamma"], t["beta"], t["W"], t["b"], t["means"], t["stdev"], S, Lp)
        grads = MR.tail_grads(t["up_y"], t["x"], t["gamma"], t["beta"], t["W"], t["stdev"], S, Lp)
    assert tuple(got.shape) == (B, Lp, C) and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for k, gr in grads.items():
        assert gr.shape == t[k].grad.shape and float((gr - t[k].grad).abs().max()) <= 1e-11 * max(1.0, float(t[k].grad.abs().max())), k
    assert bool((grads["x"][:, :S] == 0).all()) and bool((grads["x"][:, S + Lp:] == 0).all())


def test_stages_around_the_timesblock_reproduce_the_golden():
    from models.TimesNet import TimesNet
    z, params = TC.golden()
    m = TimesNet(TC.config())
    m.load_state_dict(params, strict=True)
    m = m.double().train()
    p = dict(m.named_parameters())
    tpp, data, tp, mask, up = (torch.from_numpy(z[k]).double() for k in ("tpp", "data", "tp", "mask", "upstream"))
    S, P = m.input_len, m.pred_len
    enc, means, stdev, _, _ = MR.front(data, mask, tp, tpp, S, P, p["enc_embedding.value_embedding.tokenConv.weight"],
                                       m.enc_embedding.position_embedding.pe[0], p["predict_linear.weight"], p["predict_linear.bias"])
    assert len(m.model) == 1
    enc = m.model[0](enc)
    out = MR.tail(enc, p["layer_norm.weight"], p["layer_norm.bias"], p["projection.weight"], p["projection.bias"], means.detach(),
                  stdev.detach(), S, tpp.shape[1])
    assert out.shape == z["out"].shape and TC.rel(out, z["out"]) < TC.OUT_TOL
    (out * up).sum().backward()
    want = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g.")}
    diff, errs = TC.grad_errors({k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items()}, want)
    assert not diff and max(errs.values()) < TC.GRAD_TOL, errs


def test_knob_and_exports_and_limits():
    import os
    from immtsf import _lib, config
    assert config.timesnet_model_fused is (os.environ.get("IMMTSF_TIMESNET_MODEL_FUSED", "1") != "0")
    names = {"immtsf_timesnet_model_supported", "immtsf_timesnet_front_workspace_bytes", "immtsf_timesnet_front_forward",
             "immtsf_timesnet_front_backward", "immtsf_timesnet_tail_forward", "immtsf_timesnet_tail_backward"}
    assert names <= set(_lib.exported_names())
    lib = _lib.load()
    for name, (B, L, S, Lp, P, C, D) in TC.CASES.items():
        assert lib.immtsf_timesnet_model_supported(S, P, C, D) == 1, name
        assert lib.immtsf_timesnet_front_workspace_bytes(B, S, P, C, D) > 0, name
    assert lib.immtsf_timesnet_model_supported(32, 32, 8, 16) == 1 and lib.immtsf_timesnet_model_supported(96, 96, 8, 64) == 1
    assert lib.immtsf_timesnet_model_supported(8, 4, 3, 20) == 1 and lib.immtsf_timesnet_model_supported(8, 4, 3, 18) == 0
    assert lib.immtsf_timesnet_model_supported(200, 57, 3, 8) == 0 and lib.immtsf_timesnet_model_supported(0, 4, 3, 8) == 0
    assert lib.immtsf_timesnet_model_supported(8, 4, 11, 8) == 0 and lib.immtsf_timesnet_front_workspace_bytes(2, 8, 4, 11, 8) == 0
    from models.TimesNet import TimesNet
    assert TimesNet(TC.config()).fused_calls == 0
