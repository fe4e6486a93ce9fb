"""tests/informer_ref.py (the float64 restatement of Informer's layers) pinned to the goldens the unmodified reference wrote
(tests/golden/make_golden_informer.py).  CPU only."""
import numpy as np
import pytest
import torch

import informer_cases as IC
import informer_ref as R

TOL = 1e-5      # float64 restatement against the reference's fp32 run


def _run(name):
    z, params, none, samples = IC.golden(name)
    p = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in params.items()}
    batch = [torch.from_numpy(z[k]).double() for k in ("tpp", "data", "tp", "mask")]
    out, after, gaps = R.informer(p, IC.FIXTURES[name], *batch, samples)
    (out * torch.from_numpy(z["upstream"]).double()).sum().backward()
    return z, p, none, out, after, gaps


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_restatement_meets_the_reference(name):
    z, p, none, out, after, gaps = _run(name)
    assert IC.rel(out, z["out"]) < TOL
    want = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g.")}
    assert want and all("temporal_embedding" in k for k in none)      # x_mark is None: the temporal tables take no gradient
    diff, errs = IC.grad_errors({k: p[k].grad for k in want}, want)
    assert not diff and max(errs.values()) < 10 * TOL, (diff, max(errs, key=errs.get), max(errs.values()))
    for k in (k for k in z.files if k.startswith("after.")):
        assert IC.rel(after[k[6:]], z[k]) < TOL, k
    rec = z["gap"]
    assert len(gaps) == len(rec) and float(np.min(rec)) >= 1e-3
    for a, b in zip(gaps, rec):
        assert (np.isinf(a) and np.isinf(b)) or abs(a - b) < 1e-4, (gaps, rec)


def test_fixture_shapes_take_the_branches_the_issue_names():
    z, _, _, samples = IC.golden("model_informer")
    assert z["data"].shape == (3, 10, 3) and z["tpp"].shape == (3, 4)                      # both paddings: 10 < 12, 4 < 5
    assert [tuple(s.shape) for s in samples] == [(12, 3), (7, 2), (5, 2), (5, 2)]          # u = 3 < 12; the cross-attention sees 7 keys
    assert R.n_sample(1, 12) == 3 and R.n_sample(1, 7) == 2
    z, _, _, samples = IC.golden("model_informer_nodistil")
    assert z["data"].shape == (3, 12, 3)
    assert [tuple(s.shape) for s in samples] == [(12, 9)] * 3 + [(5, 5), (5, 9)] and R.n_sample(3, 5) == 5


@pytest.mark.parametrize("case", sorted(IC.CONV_CASES))
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_conv_layer_restatement(case, mode):
    z = np.load(IC.GOLDEN + "/layer_conv_distil.npz")
    p = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in IC.conv_params(z, case).items()}
    x = torch.from_numpy(z[f"{case}.x"]).double().requires_grad_(True)
    assert tuple(x.shape) == IC.CONV_CASES[case]
    out, after = R.conv_layer(x, p, "", mode == "train")
    assert IC.rel(out, z[f"{case}.{mode}.out"]) < TOL
    (out * torch.from_numpy(z[f"{case}.{mode}.upstream"]).double()).sum().backward()
    # the golden is the reference's fp32 run, and BatchNorm over B (L + 2) = 4 rows amplifies its rounding (downConv.bias takes a zero
    # gradient through batch statistics: fp32 leaves noise there): the project's fp32 gradient bar, relative to the largest gradient
    names = ("downConv.weight", "downConv.bias", "norm.weight", "norm.bias")
    want = {k: torch.from_numpy(z[f"{case}.{mode}.g.{k}"]) for k in names}
    want["x"] = torch.from_numpy(z[f"{case}.{mode}.gx"])
    got = {**{k: p[k].grad for k in names}, "x": x.grad}
    if mode == "train":      # batch statistics remove the bias: its gradient is zero analytically, rounding noise in either run
        gmax = max(float(w.abs().max()) for w in want.values())
        assert float(got["downConv.bias"].abs().max()) < 1e-4 * gmax and float(want.pop("downConv.bias").abs().max()) < 1e-4 * gmax
    diff, errs = IC.grad_errors(got, want)
    assert not diff and max(errs.values()) < IC.GRAD_TOL, errs
    if mode == "train":
        for k, v in after.items():
            assert IC.rel(v, z[f"{case}.after.norm.{k}"]) < TOL, k


def test_ties_go_to_the_lower_index_and_repeated_keys_count_twice():
    M = torch.tensor([[[1.0, 3.0, 3.0, 0.5, 3.0]]])
    assert R.select(M, 2).tolist() == [[[1, 2]]]
    q, k = torch.ones(1, 1, 1, 2, dtype=torch.float64), torch.tensor([[[[1.0, 0.0]], [[0.0, 2.0]]]], dtype=torch.float64)
    assert float(R.measure(q, k, torch.tensor([[1, 1]]))) == 2.0 - 4.0 / 2
