"""GPU parity of the CRU and LatentODE forms of the device-side batch builder: ResidentStore.collate(form=...)
against the batches the REAL reference's loaders and its `variable_time_collate_fn_ODE` produced (tests/golden/collate_{cru,ode,
ode_edge}.npz) -- every tensor equal in shape, dtype and bits -- and, end to end, the two backbones fed from it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import collate_forms_ref as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ["data_to_predict", "mask_predicted_data", "observed_data", "observed_mask", "observed_tp", "tp_to_predict"]
FORM = {"collate_cru": "cru", "collate_ode": "ode"}
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _loader_store(name, dev):
    """(fixture, store) of a loader fixture, built once: the reference dataset's chunk list through from_chunks"""
    if name not in _cache:
        from immtsf.data import ResidentStore
        from oracle import collate_ref as R
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        zs = np.load(os.path.join(GOLDEN, "collate_standard.npz"))
        emb = {int(k[8:10]): torch.from_numpy(zs[k]) for k in zs.files if k.startswith("file.ent") and k.endswith("/emb")}
        chunks = []
        for c in R.chunks_from_golden(z):
            texts = [(float(t), emb[int(e)][int(r)]) for t, e, r in zip(c["note_t"], c["note_ent"], c["note_row"])]
            chunks.append((c["id"], torch.from_numpy(c["tt"]), torch.from_numpy(c["vals"]), torch.from_numpy(c["mask"]), texts))
        _cache[name] = (z, ResidentStore.from_chunks(chunks, float(z["history"]), float(z["pred_window"]), dev))
    return _cache[name]


def _edge_store(chunks, z, dev):
    """a store of hand-made windows; each gets one note (a store keeps at least one), which the six tensors do not depend on"""
    from immtsf.data import ResidentStore
    emb = torch.arange(8, dtype=torch.float32).reshape(2, 4)
    full = [(f"w{i}", torch.from_numpy(t), torch.from_numpy(v), torch.from_numpy(m), [(1.0 + i, emb[i % 2])]) for i, (t, v, m) in enumerate(chunks)]
    return ResidentStore.from_chunks(full, float(z["history"]), float(z["pred_window"]), dev)


def _same(got, exp):
    g = got.cpu().numpy()
    return g.shape == exp.shape and g.dtype == exp.dtype and np.array_equal(g, exp)


@pytest.mark.parametrize("name", ["collate_cru", "collate_ode"])
def test_forms_bit_exact_vs_reference_batches(name):
    z, store = _loader_store(name, _dev())
    for b in range(int(z["n_batches"])):
        got = store.collate(z[f"b{b}.window_ids"], form=FORM[name])
        keys = [k[len(f"b{b}."):] for k in z.files if k.startswith(f"b{b}.") and not k.endswith("window_ids")]
        assert sorted(keys) == sorted(SIX + ["tau", "notes_embeddings"])
        for k in keys:
            assert _same(got[k], z[f"b{b}.{k}"]), (name, b, k)
        for k in ("note_lengths", "note_offsets", "note_rowmap", "notes_packed"):      # the multimodal part, as in every form
            assert k in got


def test_ode_edge_batches_bit_exact_vs_reference():
    dev = _dev()
    z = np.load(os.path.join(GOLDEN, "collate_ode_edge.npz"))
    for name, (chunks, ids, want) in F.edge_cases(z).items():
        got = _edge_store(chunks, z, dev).collate(ids, form="ode")
        for k in SIX:
            assert _same(got[k], want[k]), (name, k)
        assert got["tau"].shape == (len(ids), 1)


def test_ode_axis_over_several_blocks_matches_restatement():
    """an axis of some thousand points, five channels (rows of 20 bytes): more than one block per window in both halves, equal
    times inside a window and between windows; against the restatement, which tests/test_collate_forms_ref.py pins to the reference"""
    dev = _dev()
    rng = np.random.default_rng(5)
    chunks = []
    for n in (700, 412, 1, 633, 520):
        t = np.sort(rng.integers(0, 4800, size=n)).astype(np.float32) * np.float32(0.01)       # a grid of 0.01 over [0, 48)
        m = (rng.random((n, 5)) < 0.7).astype(np.float32)
        chunks.append((t, rng.normal(size=(n, 5)).astype(np.float32) * m, m))
    z = {"history": 24.0, "pred_window": 24.0}
    ids = [4, 0, 2, 1, 3, 0]
    want = F.ode_collate([chunks[i] for i in ids], 24.0, 48.0)
    assert want["observed_tp"].shape[0] * 5 > 2 * 1024 and want["tp_to_predict"].shape[0] * 5 > 2 * 1024
    got = _edge_store(chunks, z, dev).collate(ids, form="ode")
    for k in SIX:
        assert _same(got[k], want[k]), k


def test_default_form_is_the_standard_collate():
    z, store = _loader_store("collate_ode", _dev())
    ids = z["b1.window_ids"]
    for patch in (None, (8, 3, 8)):
        a, b = store.collate(ids, patch=patch), store.collate(ids, patch=patch, form="standard")
        assert list(a) == list(b)
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    lean = store.collate(ids, padded_notes=False, form="ode")
    assert "notes_embeddings" not in lean and torch.equal(lean["tau"], store.collate(ids)["tau"])


def test_form_errors():
    z, store = _loader_store("collate_ode", _dev())
    with pytest.raises(ValueError):
        store.collate([0, 1], form="patch")
    for form in ("cru", "ode"):
        with pytest.raises(ValueError):
            store.collate([0, 1], patch=(8, 3, 8), form=form)
    with pytest.raises(IndexError):
        store.collate([store.W], form="ode")


def test_empty_batch_shapes():
    z, store = _loader_store("collate_ode", _dev())
    e = store.collate([], form="ode")
    assert e["observed_tp"].shape == (0,) and e["tp_to_predict"].shape == (0,)
    for k in ("observed_data", "observed_mask", "data_to_predict", "mask_predicted_data"):
        assert e[k].shape == (0, 0, store.C) and e[k].dtype == torch.float32
    assert e["note_offsets"].cpu().tolist() == [0] and e["tau"].shape == (0, 0)
    e = store.collate([], form="cru")
    assert e["observed_tp"].shape == (0, 0) and e["observed_data"].shape == (0, 0, store.C) and e["tp_to_predict"].shape == (0, 0)


def _union_into_offset_buffers(store, ids, dev):
    """immtsf_collate_union called directly, every output one float into its buffer: no base is 16-byte aligned"""
    from immtsf import _lib
    lib = _lib.load()
    axis, n_obs = store._union_axis(np.asarray(ids, dtype=np.int32))
    B, T, Cn = len(ids), len(axis), store.C
    shapes = {"observed_tp": (n_obs,), "observed_data": (B, n_obs, Cn), "observed_mask": (B, n_obs, Cn),
              "tp_to_predict": (T - n_obs,), "data_to_predict": (B, T - n_obs, Cn), "mask_predicted_data": (B, T - n_obs, Cn)}
    buf = {k: torch.full((int(np.prod(s)) + 1,), -7.0, device=dev) for k, s in shapes.items()}
    out = {k: buf[k][1:] for k in buf}
    assert all(v.data_ptr() % 16 == 4 for v in out.values())
    ids_dev = torch.tensor(ids, dtype=torch.int32, device=dev)
    axis_dev = torch.from_numpy(axis).to(dev)
    _lib.check(lib.immtsf_collate_union(C.byref(store._struct), _lib.ptr(ids_dev), B, _lib.ptr(axis_dev), T, n_obs, float(store.time_max),
                                        *[_lib.ptr(out[k]) for k in ("observed_tp", "observed_data", "observed_mask", "tp_to_predict",
                                                                    "data_to_predict", "mask_predicted_data")], _lib.stream_ptr()),
               "collate_union")
    assert all(float(buf[k][0]) == -7.0 for k in buf)           # the float in front of each output is untouched
    return {k: out[k].reshape(shapes[k]) for k in out}


def test_union_kernel_on_misaligned_outputs():
    dev = _dev()
    z = np.load(os.path.join(GOLDEN, "collate_ode_edge.npz"))
    chunks, ids, want = F.edge_cases(z)["four_channels"]        # rows of 16 bytes: aligned outputs always take the 16-byte path
    got = _union_into_offset_buffers(_edge_store(chunks, z, dev), ids, dev)
    for k in SIX:
        assert _same(got[k], want[k]), k
    z, store = _loader_store("collate_ode", dev)
    slabs = [(b, z[f"b{b}.observed_data"].shape[1] * store.C) for b in range(int(z["n_batches"]))]
    b = next(b for b, n in slabs if n % 4 == 0)                 # a loader batch whose observed slab is a whole number of 16 bytes
    got = _union_into_offset_buffers(store, [int(i) for i in z[f"b{b}.window_ids"]], dev)
    for k in SIX:
        assert _same(got[k], z[f"b{b}.{k}"]), (b, k)


def test_union_entry_point_checks_its_arguments():
    from immtsf import _lib
    dev = _dev()
    lib = _lib.load()
    z, store = _loader_store("collate_ode", dev)
    ids = torch.zeros(2, dtype=torch.int32, device=dev)
    x = torch.zeros(64, device=dev)
    st, p, s = C.byref(store._struct), _lib.ptr(x), _lib.stream_ptr()
    einval = lib.immtsf_collate_union(None, _lib.ptr(ids), 2, p, 4, 2, 48.0, p, p, p, p, p, p, s)
    assert einval < 0
    assert lib.immtsf_collate_union(st, _lib.ptr(ids), 2, p, 4, 5, 48.0, p, p, p, p, p, p, s) == einval          # n_obs > T
    assert lib.immtsf_collate_union(st, _lib.ptr(ids), 2, None, 4, 2, 48.0, p, p, p, p, p, p, s) == einval       # no axis
    assert lib.immtsf_collate_union(st, _lib.ptr(ids), 2, p, 4, 2, 48.0, p, None, p, p, p, p, s) == einval       # a half that is written
    assert lib.immtsf_collate_union(st, _lib.ptr(ids), -1, p, 4, 2, 48.0, p, p, p, p, p, p, s) == einval
    assert lib.immtsf_collate_union(st, _lib.ptr(ids), 0, p, 4, 2, 48.0, p, p, p, p, p, p, s) == 0               # B == 0: no launch


def _uploaded(z, b, dev):
    return {k: torch.from_numpy(z[f"b{b}.{k}"]).to(dev) for k in SIX}


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_latent_ode_forecasts_from_the_device_batch():
    """LatentODE.forecasting on the `ode` dict == on the same batch uploaded from the fixture, bit for bit (same seed, eval mode)"""
    import latent_ode_cases as L
    dev = _dev()
    z, store = _loader_store("collate_ode", dev)
    m = L.make_model(dev, (4, store.C, None, None, L.SMALL)).eval()
    for b in (0, int(z["n_batches"]) - 1):
        outs = []
        for batch in (store.collate(z[f"b{b}.window_ids"], form="ode"), _uploaded(z, b, dev)):
            torch.manual_seed(11)
            with torch.no_grad():
                outs.append(m.forecasting(batch["tp_to_predict"], batch["observed_data"], batch["observed_tp"], batch["observed_mask"]))
        assert outs[0].shape == z[f"b{b}.data_to_predict"].shape
        assert _bits_equal(outs[0], outs[1]), b


def test_cru_forecasts_from_the_device_batch():
    """CRU.forecasting on the `cru` dict == on the same batch uploaded from the fixture, bit for bit (eval mode)"""
    import cru_cases as K
    dev = _dev()
    z, store = _loader_store("collate_cru", dev)
    case = (4, store.C) + K.CASES["b_lsd8"][2:]
    m = K.make_model(dev, case).eval()
    for b in (0, int(z["n_batches"]) - 1):
        outs = []
        for batch in (store.collate(z[f"b{b}.window_ids"], form="cru"), _uploaded(z, b, dev)):
            torch.manual_seed(11)
            with torch.no_grad():
                outs.append(m.forecasting(batch["tp_to_predict"], batch["observed_data"], batch["observed_tp"], batch["observed_mask"]))
        assert outs[0].shape == z[f"b{b}.data_to_predict"].shape
        assert _bits_equal(outs[0], outs[1]), b
