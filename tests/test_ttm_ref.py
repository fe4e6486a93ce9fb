"""CPU checks of the TTM backbone's yardstick, module layout and ABI surface: the float64 restatement (tests/ttm_ref.py) against the real
reference's goldens (model_ttm*.npz, written by tests/golden/make_golden_ttm.py) to 1e-5, every gradient included; the product module's
state-dict keys and shapes and what its constructor writes back into `configs`; the header and the ctypes binding on the new symbols; the
library's limit and workspace queries (host arithmetic)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ttm_cases as TC  # noqa: E402
import ttm_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["immtsf_ttm_gate_backward", "immtsf_ttm_gate_forward", "immtsf_ttm_mixer_backward", "immtsf_ttm_mixer_forward",
       "immtsf_ttm_mixer_supported", "immtsf_ttm_mixer_workspace_bytes"]


@pytest.mark.parametrize("name", sorted(TC.FIXTURES))
def test_restatement_matches_reference_golden(name):
    z, params, none = TC.golden(name)
    out, grads = R.run(params, z["data"], z["mask"], z["tp"], z["upstream"], TC.FIXTURES[name])
    assert tuple(out.shape) == z["out"].shape
    assert float((out - torch.from_numpy(z["out"]).double()).abs().max()) < 1e-5
    assert {k for k, g in grads.items() if g is None} == none == set()      # every parameter of a TTM has a gradient
    assert sorted("g." + k for k in grads) == sorted(f for f in z.files if f.startswith("g."))
    for k, g in grads.items():
        assert float((g - torch.from_numpy(z["g." + k]).double()).abs().max()) < 1e-5, k


@pytest.mark.parametrize("name", sorted(TC.FIXTURES))
def test_product_module_has_the_goldens_state_dict(name):
    from models.TTM import TTM
    z, params, none = TC.golden(name)
    opts = TC.FIXTURES[name]
    cfg = TC.config(opts)
    m = TTM(cfg)
    sd = m.state_dict()
    assert sorted(sd) == sorted(params)
    for key, v in sd.items():
        assert tuple(v.shape) == tuple(params[key].shape), key
    assert cfg.n_vars == 2 * opts["enc_in"] + 1 and cfg.num_patches == TC.PATCHES[name] == R.num_patches(opts)
    assert m.immtsf_graphable and m.fused_blocks == 0
    assert tuple(m.zeros_pad.shape) == (4, max(opts["input_len"], opts["pred_len"]), opts["enc_in"])
    assert any(".patch_mixer." in k for k in sd) == (TC.PATCHES[name] > 1)
    assert any(".channel_feature_mixer." in k for k in sd) == (opts["mode"] == "mix_channel")
    assert any(k.startswith("decoder.") for k in sd) == bool(opts["use_decoder"])


def test_layers_module_mirrors_the_reference_names():
    import layers.MLP as L
    import models.TTM as T
    for n in ("TTMGatedLayer", "TTMMLP", "TTMMixerBlock", "TTMLayer"):
        assert hasattr(L, n), n
    for n in ("TTMAPBlock", "TTMBlock", "TTMPredicationHead", "TTMBackbone", "Model", "TTM"):
        assert hasattr(T, n), n
    assert issubclass(T.TTM, T.Model)
    lay = L.TTMLayer(d_model=8, num_patches=1, n_vars=5, mode="common_channel", dropout=0.0)
    assert not hasattr(lay, "patch_mixer") and not hasattr(lay, "channel_feature_mixer")


def test_header_and_binding_agree_on_the_new_symbols():
    from immtsf import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "immtsf.h")).read(), flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(immtsf_[a-z0-9_]+)\s*\(", src)) if n.startswith("immtsf_ttm_"))
    assert declared == NEW
    assert sorted(n for n in _lib.exported_names() if n.startswith("immtsf_ttm_")) == NEW
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n), n
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, src, flags=re.S).group(1)
        assert len(_lib._PROTOS[n][1]) == len([a for a in decl.split(",") if a.strip()]), n      # one ctypes entry per C argument
    assert lib.immtsf_abi_version() == _lib.ABI_VERSION


def test_supported_and_workspace_queries_run_without_gpu():
    from immtsf import _lib, config
    lib = _lib.load()
    sup, ws = lib.immtsf_ttm_mixer_supported, lib.immtsf_ttm_mixer_workspace_bytes      # mode, outer, inner, F, D
    assert sup(0, 64 * 17, 1, 8, 256) == 1 and sup(1, 64, 2, 17, 1024) == 1             # the defaults' blocks
    assert sup(0, 1, 1, 2, 1) == 1 and sup(0, 3, 1, 32, 64) == 1 and sup(1, 1, 1, 32, 65536) == 1
    assert sup(0, 3, 1, 33, 64) == 0 and sup(1, 3, 2, 33, 64) == 0 and sup(0, 3, 1, 0, 64) == 0
    assert sup(0, 3, 2, 8, 64) == 0                     # patch mode has no inner axis
    assert sup(2, 3, 1, 8, 64) == 0 and sup(0, 0, 1, 8, 64) == 0 and sup(0, 3, 1, 8, 0) == 0 and sup(0, 3, 1, 8, 65537) == 0
    assert sup(0, 2 ** 31 // (8 * 64), 1, 8, 64) == 0 and sup(0, 2 ** 31 // (8 * 64) - 1, 1, 8, 64) == 1      # 2^31 elements
    nv = lambda F, D: 5 * F * F + 4 * F + 2 * D      # noqa: E731
    assert ws(0, 5, 1, 8, 3) == 1 * nv(8, 3) * 4 + 256                  # 16 groups of 3 columns per chunk: one chunk, one slab
    assert ws(1, 64, 2, 17, 1024) == 128 * nv(17, 1024) * 4 + 256       # a group per chunk
    assert ws(1, 4096, 8, 17, 256) == 512 * nv(17, 256) * 4 + 256       # never more slabs than 512
    assert ws(0, 3, 1, 33, 64) == 0
    assert ws(1, 2 ** 14, 1, 32, 65536) <= (32 << 20) + 256             # fewer workgroups, not more memory
    assert isinstance(config.ttm_fused, bool)


def test_restatement_block_takes_masks_in_the_kernels_element_order():
    """one channel-mode block by hand, entry by entry: the group of (b, n) is b N + n, and k1[g, c, j] / k2[g, c, o] multiply the hidden
    value j / the mixed value o of that group's column c -- a transposed or mis-strided mask layout in the restatement fails here, in the
    output and in dx (central differences through the hand computation)"""
    import math
    B, M, N, D = 2, 3, 2, 2
    x, up, params = TC.block_tensors(B, M, N, D, "channel", seed=4)
    g = torch.Generator().manual_seed(9)
    k1 = (torch.rand(B * N, D, 2 * M, generator=g) < 0.6).double() * 2.5
    k2 = (torch.rand(B * N, D, M, generator=g) < 0.6).double() * 2.5
    assert 0 < float(k1.eq(0).double().mean()) < 1 and 0 < float(k2.eq(0).double().mean()) < 1
    gamma, beta, W1, b1, W2, b2, Wg, bg = [p.double() for p in params]

    def by_hand(xd):
        out = xd.clone()
        mu = xd.mean(-1, keepdim=True)
        xn = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * gamma + beta
        for b in range(B):
            for n in range(N):
                for c in range(D):
                    v = [float(xn[b, f, n, c]) for f in range(M)]
                    h = []
                    for j in range(2 * M):
                        a = float(b1[j]) + sum(float(W1[j, f]) * v[f] for f in range(M))
                        h.append(0.5 * a * (1 + math.erf(a / math.sqrt(2))) * float(k1[b * N + n, c, j]))
                    u = [(float(b2[o]) + sum(float(W2[o, j]) * h[j] for j in range(2 * M))) * float(k2[b * N + n, c, o]) for o in range(M)]
                    z = [float(bg[o]) + sum(float(Wg[o, f]) * u[f] for f in range(M)) for o in range(M)]
                    e = [math.exp(t - max(z)) for t in z]
                    for f in range(M):
                        out[b, f, n, c] += u[f] * e[f] / sum(e)
        return out
    out, dx, _ = R.run_block(x, params, up, "channel", keep=(k1, k2))
    assert float((out - by_hand(x.double())).abs().max()) < 1e-12
    for idx in [(0, 0, 0, 0), (1, 2, 1, 1), (0, 1, 1, 0)]:
        hi, lo = x.double().clone(), x.double().clone()
        hi[idx] += 1e-5
        lo[idx] -= 1e-5
        num = float(((by_hand(hi) - by_hand(lo)) * up.double()).sum()) / 2e-5
        assert abs(num - float(dx[idx])) < 1e-6 * max(1.0, abs(num)), idx
