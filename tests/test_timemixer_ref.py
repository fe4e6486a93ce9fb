"""CPU checks of the TimeMixer backbone's yardstick, module layout and limits: the float64 restatement (tests/timemixer_ref.py) against the
real reference's goldens (model_timemixer.npz, model_timemixer_odd.npz, written by tests/golden/make_golden_timemixer.py) to 1e-5,
gradients and the set of gradient-less parameters included; the product module's state-dict keys and shapes; the library's limit and
workspace queries (host arithmetic); and the margin of the GPU tests' bars -- torch's own fp32 CPU run of the restatement must sit at
least 4x inside them on every shape of the GPU parity list."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import timemixer_cases as TC  # noqa: E402
import timemixer_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {      # name: C, input_len, pred_len, d_model, d_ff, e_layers, moving_avg
    "model_timemixer": (3, 8, 6, 8, 12, 2, 5),
    "model_timemixer_odd": (3, 33, 7, 16, 32, 2, 25),
}


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    params = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p.")}
    none = set(str(z["none"]).split("\n"))
    return z, params, none


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_restatement_matches_reference_golden(name):
    C, S, P, d, dff, E, k = FIXTURES[name]
    z, params, none = _golden(name)
    out, grads = R.run(params, z["data"], z["mask"], z["tp"], z["upstream"], S, P, E, k)
    assert tuple(out.shape) == z["out"].shape
    assert float((out - torch.from_numpy(z["out"]).double()).abs().max()) < 1e-5
    assert {k_ for k_, g in grads.items() if g is None} == none
    n = len(R.scale_lengths(S, 3)) - 1
    assert none == R.dead_names(grads.keys(), E, n)
    live = [k_ for k_ in grads if k_ not in none]
    assert sorted("g." + k_ for k_ in live) == sorted(f for f in z.files if f.startswith("g."))
    for k_ in live:      # 1e-5 absolute, as for the output (the largest gradients are 4.3 and 12.3)
        assert float((grads[k_] - torch.from_numpy(z["g." + k_]).double()).abs().max()) < 1e-5, k_
    assert sum(int(np.prod(z["g." + k_].shape)) for k_ in live) > 0


def test_live_parameter_count_at_the_reference_defaults():
    """input_len = pred_len = 24, C = 3, d_model 16, d_ff 32, e_layers 2: 7 449 parameters, 5 063 of them with a gradient"""
    from models.TimeMixer import TimeMixer
    m = TimeMixer(TC.config(3, 24, 24, 16, 32, 2, 25, batch_size=4))
    names = dict(m.named_parameters())
    dead = R.dead_names(names, 2, m.down_layers)
    assert sum(p.numel() for p in names.values()) == 7449
    assert sum(p.numel() for k, p in names.items() if k not in dead) == 5063
    from immtsf import _lib
    assert _lib.load().immtsf_timemixer_grad_layout(24, 24, 3, 16, 32, 2, 3, None, 0) == 5063


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_product_module_has_the_goldens_state_dict(name):
    from models.TimeMixer import TimeMixer
    C, S, P, d, dff, E, k = FIXTURES[name]
    z, params, none = _golden(name)
    cfg = TC.config(C, S, P, d, dff, E, k, batch_size=4)
    m = TimeMixer(cfg)
    sd = m.state_dict()
    assert sorted(sd) == sorted(params)
    for key, v in sd.items():
        want = tuple(params[key].shape)
        got = tuple(v[:, :S].shape) if key.endswith(".pe") else tuple(v.shape)
        assert got == want, key
    assert cfg.down_sampling_layers == 3 and m.immtsf_graphable and m.fused_calls == 0
    assert {k_ for k_ in dict(m.named_parameters())} - none == {f[2:] for f in z.files if f.startswith("g.")}
    np.testing.assert_allclose(sd["enc_embedding.position_embedding.pe"][:, :S].numpy(), params["enc_embedding.position_embedding.pe"].numpy(),
                               atol=1e-6)


@pytest.mark.parametrize("S,lengths", [(3, [3, 1]), (6, [6, 3, 1]), (8, [8, 4, 2, 1]), (33, [33, 16, 8, 4])])
def test_short_inputs_clip_the_pyramid_in_place(S, lengths):
    from models.TimeMixer import TimeMixer
    cfg = TC.config(3, S, 4, 8, 12, 2, 5, batch_size=4)
    m = TimeMixer(cfg)
    n = len(lengths) - 1
    assert R.scale_lengths(S, 3) == lengths
    assert cfg.down_sampling_layers == n == m.down_layers      # written back into the caller's configs
    sd = m.state_dict()
    assert len(m.predict_layers) == n + 1 and len(m.normalize_layers) == n + 1
    for i in range(n + 1):
        assert tuple(sd[f"predict_layers.{i}.weight"].shape) == (4, lengths[i])
        assert tuple(sd[f"normalize_layers.{i}.affine_weight"].shape) == (3,)
    for j in range(2):
        for i in range(n):
            a, b = lengths[i], lengths[i + 1]
            assert tuple(sd[f"pdm_blocks.{j}.mix_season.down_sampling_layers.{i}.0.weight"].shape) == (b, a)
            assert tuple(sd[f"pdm_blocks.{j}.mix_season.down_sampling_layers.{i}.2.weight"].shape) == (b, b)
            assert tuple(sd[f"pdm_blocks.{j}.mix_trend.up_sampling_layers.{n - 1 - i}.0.weight"].shape) == (a, b)
            assert tuple(sd[f"pdm_blocks.{j}.mix_trend.up_sampling_layers.{n - 1 - i}.2.weight"].shape) == (a, a)
        assert f"pdm_blocks.{j}.mix_season.down_sampling_layers.{n}.0.weight" not in sd
        assert f"pdm_blocks.{j}.cross_layer.0.weight" not in sd
    assert tuple(sd["enc_embedding.value_embedding.tokenConv.weight"].shape) == (8, 7, 3)
    assert "pdm_blocks.0.cross_layer.0.weight" in TimeMixer(TC.config(3, S, 4, 8, 12, 2, 5, batch_size=4, channel_independence=0)).state_dict()


def test_option_values_outside_the_fused_path_are_rejected_before_the_library_is_asked():
    """the Python half of the limits (TimeMixer._fused_dims): window 3, another pooling or decomposition, channel dependence -> None"""
    from models.TimeMixer import TimeMixer
    assert TimeMixer(TC.config(5, 24, 24, 16, 32, 2, 25, batch_size=4))._fused_dims() == (24, 24, 5, 16, 32, 2, 3, 25)
    assert TimeMixer(TC.config(5, 27, 24, 16, 32, 2, 25, batch_size=4, down_sampling_window=3))._fused_dims() is None
    for over in (dict(down_sampling_method="max"), dict(down_sampling_method="conv"), dict(decomp_method="dft_decomp", top_k=2),
                 dict(channel_independence=0)):
        assert TimeMixer(TC.config(5, 24, 24, 16, 32, 2, 25, batch_size=4, **over))._fused_dims() is None, over


def test_supported_and_workspace_queries_run_without_gpu():
    from immtsf import _lib
    lib = _lib.load()
    sup = lib.immtsf_timemixer_supported      # S, P, C, d_model, d_ff, e_layers, down_layers, moving_avg
    assert sup(24, 24, 5, 16, 32, 2, 3, 25) == 1
    assert sup(64, 64, 31, 32, 64, 4, 6, 25) == 1 and sup(64, 64, 3, 32, 64, 4, 3, (1 << 24) - 1) == 1      # the corner
    assert sup(2, 1, 1, 1, 1, 1, 1, 1) == 1 and sup(3, 4, 3, 8, 12, 2, 1, 5) == 1
    assert sup(65, 24, 5, 16, 32, 2, 3, 25) == 0 and sup(24, 65, 5, 16, 32, 2, 3, 25) == 0
    assert sup(24, 24, 5, 33, 32, 2, 3, 25) == 0 and sup(24, 24, 5, 16, 65, 2, 3, 25) == 0
    assert sup(24, 24, 5, 16, 32, 5, 3, 25) == 0 and sup(24, 24, 5, 16, 32, 0, 3, 25) == 0
    assert sup(24, 24, 32, 16, 32, 2, 3, 25) == 0      # 2C+1 = 65
    assert sup(24, 24, 5, 16, 32, 2, 3, 24) == 0 and sup(24, 24, 5, 16, 32, 2, 3, 0) == 0      # even / empty windows
    assert sup(1, 24, 5, 16, 32, 2, 0, 25) == 0 and sup(24, 24, 5, 16, 32, 2, 0, 25) == 0      # one scale alone: the reference's IndexError
    assert sup(6, 4, 3, 8, 12, 2, 3, 5) == 0           # 6 >> 3 = 0: not a clipped count
    ws = lib.immtsf_timemixer_workspace_bytes      # B, S, P, C, d_model, d_ff, e_layers, down_layers
    nv = lib.immtsf_timemixer_grad_layout(24, 24, 5, 16, 32, 2, 3, None, 0)
    act = 45 * 11 + 2 * 4 * 45 * 16 + 24 * 16      # pyramid | per block 4 x [45][16] | dec
    assert ws(4, 24, 24, 5, 16, 32, 2, 3) == 4 * (nv + act) * 4 + 256
    assert ws(4096, 24, 24, 5, 16, 32, 2, 3) == 256 * (nv + act) * 4 + 256      # never more slabs than 256
    assert ws(300, 24, 24, 5, 16, 32, 2, 3) == 150 * (nv + act) * 4 + 256       # shares of two windows
    assert ws(0, 24, 24, 5, 16, 32, 2, 3) == 0 and ws(4, 65, 24, 5, 16, 32, 2, 3) == 0
    assert ws(100000, 64, 64, 31, 32, 64, 4, 6) <= (32 << 20) + 256             # the corner: fewer workgroups, not more memory
    sizes = [ws(b, 24, 24, 5, 16, 32, 2, 3) for b in (1, 2, 16, 130, 5000)]
    assert sizes == sorted(sizes) and sizes[0] > 0


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_fp32_cpu_sits_four_times_inside_the_gpu_bars(name):
    case = TC.CASES[name]
    m = TC.make_model("cpu", case)
    batch = TC.make_batch("cpu", case)
    want_out, want = TC.reference(m, case, batch)
    got_out, got = TC.reference(m, case, batch, dtype=torch.float32)
    e_out = TC.rel(got_out, want_out)
    diff, errs = TC.grad_errors(got, want)
    print(name, "out", e_out, "worst grad", max(errs.values()))
    assert not diff
    assert e_out < TC.OUT_TOL / 4
    assert max(errs.values()) < TC.GRAD_TOL / 4, max(errs, key=errs.get)
