"""tests/informer_model_ref.py (the float64 yardsticks of csrc/informer.hip) pinned: at both fixtures' inputs and parameters `front`
is the padding + normalisation + `_embed` path of tests/informer_ref.py, and `tail` behind that file's decoder output reproduces the
goldens of the unmodified reference."""
import pytest
import torch

import informer_cases as IC
import informer_model_ref as MR
import informer_ref as R


def _fixture(name):
    z, params, none, samples = IC.golden(name)
    p = {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}
    batch = tuple(torch.from_numpy(z[k]).double() for k in ("tpp", "data", "tp", "mask"))
    return z, p, samples, batch


def _front(p, opts, batch):
    tpp, data, tp, mask = batch
    return MR.front(data, mask, tp, tpp, opts["input_len"], opts["pred_len"], p["enc_embedding.value_embedding.tokenConv.weight"],
                    p["dec_embedding.value_embedding.tokenConv.weight"], p["enc_embedding.position_embedding.pe"][0],
                    p["dec_embedding.position_embedding.pe"][0])


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_front_is_the_embed_path_of_informer_ref(name):
    opts = IC.FIXTURES[name]
    z, p, _, (tpp, data, tp, mask) = _fixture(name)
    enc, dec, means, stdev = _front(p, opts, (tpp, data, tp, mask))
    B, L, C = data.shape
    zh = data.new_zeros(B, opts["input_len"] - L, C)
    d, m, t = torch.cat([data, zh], 1), torch.cat([mask, zh], 1), torch.cat([tp, zh[:, :, 0]], 1)
    tq = torch.cat([tpp, tpp.new_zeros(B, opts["pred_len"] - tpp.shape[1])], 1)
    cnt = m.sum(1, keepdim=True).clamp(min=1)
    x = d * m
    mu = x.sum(1, keepdim=True) / cnt
    x = x - mu
    sd = torch.sqrt(((x * m) ** 2).sum(1, keepdim=True) / cnt + 1e-5)
    zp = d.new_zeros(B, opts["pred_len"], C)
    want_enc = R._embed(torch.cat([x / sd, m, t.unsqueeze(-1)], -1), p, "enc_embedding.")
    want_dec = R._embed(torch.cat([zp, zp, tq.unsqueeze(-1)], -1), p, "dec_embedding.")
    for got, want in ((enc, want_enc), (dec, want_dec), (means, mu), (stdev, sd)):
        assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("name", sorted(IC.FIXTURES))
def test_tail_behind_the_decoder_of_informer_ref_reproduces_the_golden(name, monkeypatch):
    opts = IC.FIXTURES[name]
    z, p, samples, (tpp, data, tp, mask) = _fixture(name)
    seen = {}
    ln = R._ln

    def spy(x, params, pre, eps=1e-5):
        if pre == "decoder.norm.":
            seen["x"] = x
        return ln(x, params, pre, eps)
    monkeypatch.setattr(R, "_ln", spy)
    out, _, _ = R.informer(p, opts, tpp, data, tp, mask, samples)
    _, _, means, stdev = _front(p, opts, (tpp, data, tp, mask))
    got = MR.tail(seen["x"], p["decoder.norm.weight"], p["decoder.norm.bias"], p["decoder.projection.weight"], p["decoder.projection.bias"],
                  means, stdev, tpp.shape[1])
    assert float((got - out).abs().max()) < 1e-12
    assert IC.rel(got, z["out"]) < IC.OUT_TOL
