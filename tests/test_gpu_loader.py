"""GPU side of the resident loaders: lib.parse_datasets (lib/resident_datasets.py) on the seeded dataset of tests/loader_dataset.py against what the REAL
reference's parse_datasets produced on the same files (tests/golden/loader_*.npz, bit for bit), immtsf_collate_batch against the kernels
it stands in for (inside guard bands), ResidentLoader's epochs and copy counts, the device _patch_max, and one step of the zero-edit seam
on a loader batch."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import loader_dataset as D

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX = ["data_to_predict", "mask_predicted_data", "observed_data", "observed_mask", "observed_tp", "tp_to_predict"]
INDEX = ["note_lengths", "note_offsets", "note_rowmap"]
_cache = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    r = tmp_path_factory.mktemp("loader_syn")
    digest = D.write_dataset(str(r))
    assert digest == str(np.load(os.path.join(GOLDEN, "loader_meta.npz"))["csv_sha256"]), "the regenerated dataset differs from the fixture's"
    return str(r)


def _parsed(root, model):
    """(args, data_obj) of parse_datasets for one model, built once"""
    if model not in _cache:
        from lib.parse_datasets import parse_datasets
        args = D.loader_args(root, model, _dev())
        _cache[model] = (args, parse_datasets(args, show_summary=False))
    return _cache[model]


def _nine(root):
    """the 9-window store (ent00 + ent01: among them the window with one note and the window with one history row)"""
    if "nine" not in _cache:
        from immtsf.data import ResidentStore
        store, ids = ResidentStore.from_dataset_dir(os.path.join(root, "SYN"), D.HISTORY, D.PRED_WINDOW, D.STRIDE, _dev(), time_unit="hours",
                                                    llm_model_fusion="TOY16", rec_ids=D.NINE)
        assert store.W == 9 and int(store.n_notes.min()) == 1 and int(store.hist_len.min()) == 1
        _cache["nine"] = store
    return _cache["nine"]


def _same(got, exp):
    g = got.cpu().numpy()
    return g.shape == exp.shape and g.dtype == exp.dtype and np.array_equal(g, exp)


def _equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("model", D.MODELS)
def test_parse_datasets_matches_the_reference(root, model):
    from immtsf.data import ResidentLoader
    meta, z = np.load(os.path.join(GOLDEN, "loader_meta.npz")), np.load(os.path.join(GOLDEN, f"loader_{model}.npz"))
    args, res = _parsed(root, model)
    assert sorted(res) == ["ds", "input_dim", "test_dataloader", "time_max", "train_dataloader", "val_dataloader"]
    store = res["ds"].store
    assert res["ds"].chunk_ids == [str(c) for c in meta["chunk_ids"]] and len(res["ds"]) == store.W == len(meta["chunk_ids"])
    for split in ("train", "val", "test"):
        dl = res[f"{split}_dataloader"]
        assert isinstance(dl, ResidentLoader) and dl.window_ids.tolist() == meta[f"sample.{split}_idx"].tolist()
        assert len(dl.dataset) == len(meta[f"sample.{split}_idx"])
    assert res["input_dim"] == int(meta["input_dim"])
    assert res["time_max"].is_cuda and _same(res["time_max"], meta["time_max"])
    if model == "tPatchGNN":        # the defaults were written back into args
        assert [args.patch_size, args.npatch, args.patch_stride] == z["patch"].tolist()
    val = list(res["val_dataloader"])
    assert len(val) == len(res["val_dataloader"]) == 2
    torch.manual_seed(7)
    train0 = next(iter(res["train_dataloader"]))
    for name, got in (("val_first", val[0]), ("val_last", val[-1]), ("train_first", train0)):
        keys = [k[len(name) + 1:] for k in z.files if k.startswith(name + ".") and not k.endswith("window_ids")]
        assert sorted(keys) == sorted(SIX + ["tau", "notes_embeddings"])
        for k in keys:
            assert _same(got[k], z[f"{name}.{k}"]), (model, name, k)
        direct = store.collate(z[f"{name}.window_ids"], patch=res["val_dataloader"].patch, form=res["val_dataloader"].form)
        for k in INDEX:
            assert _equal(got[k], direct[k]), (model, name, k)
        assert got["note_offsets"].cpu().tolist()[-1] == got["note_rowmap"].numel() == int(got["note_lengths"].sum())


@pytest.mark.parametrize("model", D.MODELS)
def test_get_input_and_pred_len_matches_the_reference(root, model):
    from lib.parse_datasets import get_input_and_pred_len
    z = np.load(os.path.join(GOLDEN, f"loader_{model}.npz"))
    _, res = _parsed(root, model)
    store = res["ds"].store
    before = (store.launches, store.h2d_copies)
    torch.manual_seed(5)
    assert list(get_input_and_pred_len(res)) == z["input_and_pred_len"].tolist()
    assert (store.launches, store.h2d_copies) == before         # answered from host metadata: no batch was built


def test_unimodal_run_windows_by_text_csv_and_carries_no_notes(root):
    """enable_text=False: the embedding files are not read, the windows are those the raw note times choose, tau is (B, 0)"""
    from lib.parse_datasets import parse_datasets
    meta = np.load(os.path.join(GOLDEN, "loader_meta.npz"))
    res = parse_datasets(D.loader_args(root, "DLinear", _dev(), enable_text=False), show_summary=False)
    assert res["ds"].chunk_ids == [str(c) for c in meta["unimodal.chunk_ids"]]
    batch = next(iter(res["val_dataloader"]))
    assert sorted(k for k in batch if k in SIX + ["tau", "notes_embeddings", "notes_text"]) == meta["unimodal.keys"].tolist()
    assert list(batch["tau"].shape) == meta["unimodal.tau_shape"].tolist() and batch["note_rowmap"].numel() == 0
    full = np.load(os.path.join(GOLDEN, "loader_DLinear.npz"))
    for k in SIX:
        assert _same(batch[k], full[f"val_first.{k}"]), k


@pytest.mark.parametrize("model", ["tPatchGNN", "LatentODE"])
def test_unimodal_run_in_the_patch_and_ode_forms(root, model):
    """the store without notes (d_m = 0) through the forms that keep the separate note kernels: the reference's tensors, tau (B, 0)"""
    from lib.parse_datasets import parse_datasets
    res = parse_datasets(D.loader_args(root, model, _dev(), enable_text=False), show_summary=False)
    assert res["ds"].store.d_m == 0
    batches = list(res["val_dataloader"])
    full = np.load(os.path.join(GOLDEN, f"loader_{model}.npz"))
    for name, batch in (("val_first", batches[0]), ("val_last", batches[-1])):
        for k in SIX:
            assert _same(batch[k], full[f"{name}.{k}"]), (model, name, k)
        B = len(full[f"{name}.window_ids"])
        assert batch["tau"].shape == (B, 0) and "notes_embeddings" not in batch and batch["note_rowmap"].numel() == 0
        assert batch["note_lengths"].cpu().tolist() == [0] * B and batch["note_offsets"].cpu().tolist() == [0] * (B + 1)


@pytest.mark.parametrize("model", D.MODELS)
def test_device_without_an_index_as_main_py_passes_it(root, model):
    """main.py sets args.device = torch.device("cuda"); the tensors of that device report cuda:0, which is another device object"""
    from lib.parse_datasets import parse_datasets
    z = np.load(os.path.join(GOLDEN, f"loader_{model}.npz"))
    _dev()
    res = parse_datasets(D.loader_args(root, model, torch.device("cuda")), show_summary=False)
    assert res["ds"].store.device == torch.device("cuda", torch.cuda.current_device())
    val = list(res["val_dataloader"])
    torch.manual_seed(7)
    train0 = next(iter(res["train_dataloader"]))
    for name, got in (("val_first", val[0]), ("val_last", val[-1]), ("train_first", train0)):
        for k in SIX + ["tau", "notes_embeddings"]:
            assert _same(got[k], z[f"{name}.{k}"]), (model, name, k)


def test_iter_draws_and_uploads_at_once_like_a_dataloader(root):
    """iter(loader) alone leaves the RNG where iter(DataLoader) leaves it after its first batch is asked for, and has uploaded the
    ids: reseeding between iter() and next() does not change the epoch"""
    from torch.utils.data import DataLoader

    from immtsf.data import ResidentLoader
    store = _nine(root)
    dl = ResidentLoader(store, np.arange(9), 4, True)
    torch.manual_seed(77)
    want = dl.window_ids[ResidentLoader(store, np.arange(9), 4, True)._epoch_order()]
    torch.manual_seed(77)
    live = iter(DataLoader(list(range(9)), batch_size=4, shuffle=True))
    next(live)                                                   # (torch's sampler draws its seed at the first batch)
    state = torch.get_rng_state()
    torch.manual_seed(77)
    copies = dl.h2d_copies
    it = iter(dl)
    assert torch.equal(torch.get_rng_state(), state) and dl.h2d_copies == copies + 1
    torch.manual_seed(1)
    for k, batch in enumerate(it):
        direct = store.collate(want[4 * k:4 * k + 4])
        for key in SIX + ["tau", "notes_embeddings"] + INDEX:
            assert _equal(batch[key], direct[key]), key
    assert list(ResidentLoader(store, [], 4, False)) == []


def _wide_store(dev):
    """9 windows with up to 600 notes of 8 numbers: immtsf_collate_batch then runs several chunks of workgroups per window, some of
    which lie wholly behind a window's notes (n = 1, 2, 40), end inside a chunk (257, 300, 513) or on its edge (256)"""
    if "wide" not in _cache:
        from immtsf.data import ResidentStore
        rng = np.random.default_rng(3)
        counts = [1, 300, 600, 257, 256, 2, 513, 40, 600]
        tt, row_off = [], [0]
        for w in range(9):
            nh, npred = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            tt.append(np.concatenate([np.sort(rng.random(nh) * 24), 24 + np.sort(rng.random(npred) * 24)]).astype(np.float32))
            row_off.append(row_off[-1] + nh + npred)
        R, S = row_off[-1], sum(counts)
        mask = (rng.random((R, 3)) < 0.7).astype(np.float32)
        vals = rng.normal(size=(R, 3)).astype(np.float32) * mask
        tau = np.concatenate([np.sort(rng.random(n) * 24) for n in counts]).astype(np.float32)
        _cache["wide"] = ResidentStore(np.concatenate(tt), vals, mask, np.array(row_off, np.int64), tau, rng.permutation(S).astype(np.int64),
                                       np.cumsum([0] + counts).astype(np.int64), rng.normal(size=(S, 8)).astype(np.float32), 24.0, 24.0, dev)
    return _cache["wide"]


@pytest.mark.parametrize("padded_notes", [True, False])
@pytest.mark.parametrize("ids", [[2, 0, 3, 4, 8, 5, 1], [0, 5, 7], [6], [7, 6, 2, 2, 0]])
def test_collate_batch_over_several_chunks_of_workgroups(ids, padded_notes):
    store = _wide_store(_dev())
    ids = np.array(ids, dtype=np.int32)
    ids_dev = torch.from_numpy(ids).to(store.device)
    want = store.collate(ids, padded_notes=padded_notes)
    got = _collate_batch_banded(store, ids_dev, ids, "standard", padded_notes)
    for k, v in got.items():
        assert _equal(v, want[k]), k


def _banded(shape, dtype, dev, guard=64):
    """(the whole buffer, the output inside it): `guard` sentinel elements on each side of the output"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), -7, dtype=dtype, device=dev)
    return buf, buf[guard:guard + n].view(shape)


def _collate_batch_banded(store, ids_dev, ids, form, padded_notes, guard=64):
    from immtsf import _lib
    lib, dev, f32, i32 = _lib.load(), store.device, torch.float32, torch.int32
    B, Cn = len(ids), store.C
    L, Lp, N = int(store.hist_len[ids].max()), int(store.pred_len[ids].max()), int(store.n_notes[ids].max())
    shapes = {"observed_tp": ((B, L), f32), "observed_data": ((B, L, Cn), f32), "observed_mask": ((B, L, Cn), f32),
              "tp_to_predict": ((B, Lp), f32), "data_to_predict": ((B, Lp, Cn), f32), "mask_predicted_data": ((B, Lp, Cn), f32),
              "tau": ((B, N), f32), "notes_embeddings": ((B, N, store.d_m), f32), "note_lengths": ((B,), i32),
              "note_offsets": ((B + 1,), i32), "note_rowmap": ((int(store.n_notes[ids].sum()),), i32)}
    if not padded_notes:
        del shapes["notes_embeddings"]
    bufs = {k: _banded(s, dt, dev, guard) for k, (s, dt) in shapes.items()}
    out = {k: v[1] for k, v in bufs.items()}
    p = lambda k: _lib.ptr(out[k]) if k in out else None      # noqa: E731
    rc = lib.immtsf_collate_batch(C.byref(store._struct), _lib.ptr(ids_dev), B, L, Lp, N, 1.0 if form == "cru" else float(store.time_max),
                                  p("observed_tp"), p("observed_data"), p("observed_mask"), p("tp_to_predict"), p("data_to_predict"),
                                  p("mask_predicted_data"), p("tau"), p("notes_embeddings"), p("note_lengths"), p("note_offsets"),
                                  p("note_rowmap"), _lib.stream_ptr())
    assert rc == 0
    for k, (buf, _) in bufs.items():
        assert bool((buf[:guard] == -7).all()) and bool((buf[buf.numel() - guard:] == -7).all()), f"{k}: written outside the output"
    return out


# positions into the shuffled epoch buffer below: a slice at a non-zero offset; windows out of order, and one listed twice
EPOCH = [6, 2, 8, 2, 0, 7, 3, 5, 1, 4, 8]
SLICES = {1: 3, 3: 1, 5: 4}         # B -> offset: [2], [2, 8, 2], [0, 7, 3, 5, 1]


@pytest.mark.parametrize("form", ["standard", "cru"])
@pytest.mark.parametrize("padded_notes", [True, False])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_collate_batch_equals_the_separate_kernels(root, B, padded_notes, form):
    store = _nine(root)
    epoch_dev = torch.tensor(EPOCH, dtype=torch.int32, device=store.device)
    off = SLICES[B]
    ids = np.array(EPOCH[off:off + B], dtype=np.int32)
    want = store.collate(ids, padded_notes=padded_notes, form=form)
    got = _collate_batch_banded(store, epoch_dev[off:off + B], ids, form, padded_notes)
    assert ("notes_embeddings" in want) == padded_notes
    for k, v in got.items():
        assert _equal(v, want[k]), k
    via = store.collate(ids, padded_notes=padded_notes, form=form, _ids_dev=epoch_dev[off:off + B], _one_launch=True)
    assert list(via) == list(want)
    for k in want:
        if torch.is_tensor(want[k]):
            assert _equal(via[k], want[k]), k


def test_collate_batch_on_misaligned_outputs_and_bad_arguments(root):
    """every output one element off a 16-byte boundary (the embeddings then go element by element), and the entry's argument checks"""
    from immtsf import _lib
    store = _nine(root)
    ids = np.array([0, 7, 3, 5, 1], dtype=np.int32)
    ids_dev = torch.from_numpy(ids).to(store.device)
    want = store.collate(ids)
    got = _collate_batch_banded(store, ids_dev, ids, "standard", True, guard=65)
    assert got["notes_embeddings"].data_ptr() % 16 == 4
    for k, v in got.items():
        assert _equal(v, want[k]), k
    lib, st, s = _lib.load(), C.byref(store._struct), _lib.stream_ptr()
    x, n = torch.zeros(4096, device=store.device), torch.zeros(64, dtype=torch.int32, device=store.device)
    p, q, i = _lib.ptr(x), _lib.ptr(n), _lib.ptr(ids_dev)
    ok = lambda **kw: lib.immtsf_collate_batch(*[kw.get(name, val) for name, val in (      # noqa: E731
        ("st", st), ("ids", i), ("B", 5), ("L", 2), ("Lp", 2), ("N", 2), ("tm", 48.0), ("otp", p), ("od", p), ("om", p), ("ptp", p),
        ("pd", p), ("pm", p), ("tau", p), ("notes", None), ("len", q), ("off", q), ("map", q), ("s", s))])
    assert ok(st=None) < 0 and ok(ids=None) < 0 and ok(B=0) < 0 and ok(L=-1) < 0 and ok(od=None) < 0 and ok(pm=None) < 0
    assert ok(tau=None) < 0 and ok(map=None) < 0 and ok(len=None) < 0 and ok(off=None) < 0


@pytest.mark.parametrize("form,patch", [("standard", None), ("cru", None), ("standard", (8, 3, 8)), ("ode", None)])
def test_epoch_visits_every_window_once_with_one_id_upload(root, form, patch):
    from immtsf.data import ResidentLoader
    store = _nine(root)
    dl = ResidentLoader(store, np.arange(9), 4, True, form=form, patch=patch)
    assert len(dl) == 3 and len(dl.dataset) == 9
    for epoch in (1, 2):
        torch.manual_seed(40 + epoch)
        want = dl.window_ids[ResidentLoader(store, np.arange(9), 4, True)._epoch_order()]
        torch.manual_seed(40 + epoch)
        copies, launches, sizes = dl.h2d_copies, dl.launches, []
        for k, batch in enumerate(dl):
            ids = want[4 * k:4 * k + 4]
            direct = store.collate(ids, patch=patch, form=form)
            assert list(batch) == list(direct)
            for key in direct:
                if torch.is_tensor(direct[key]):
                    assert _equal(batch[key], direct[key]), (form, key)
            sizes.append(int(batch["tau"].shape[0]))
        assert sizes == [4, 4, 1] and sorted(want.tolist()) == list(range(9))
        per_batch = {"ode": 1}.get(form, 0)                     # the ODE form's time axis is data and still goes over per batch
        assert dl.h2d_copies - copies == 1 + 3 * per_batch
        if patch is None and form != "ode":
            assert dl.launches - launches == 3                  # one launch per batch


@pytest.mark.parametrize("key", [(4, 5, 4), (1, 6, 1)])
def test_patch_max_on_the_device_equals_the_host_loop(root, key):
    """(1, 6, 1): one-hour patches over [0, 5) and a last one up to `history` -- most windows have patches that hold nothing"""
    _, res = _parsed(root, "tPatchGNN")
    store = res["ds"].store
    store._patch_cache.pop(key, None)
    want = store._patch_max_host(*key)
    got = store._patch_max(*key)
    assert got.dtype == np.int32 and got.shape == (store.W,) and np.array_equal(got, want)
    assert want.min() >= 1 and want.max() > want.min()
    if key == (1, 6, 1):
        a = store._row_off[:-1]
        empty = [not ((store._tt[a[w]:a[w] + store.hist_len[w]] >= 1) & (store._tt[a[w]:a[w] + store.hist_len[w]] < 2)).any() for w in range(store.W)]
        assert any(empty)
    assert store._patch_max(*key) is got                        # cached: one kernel and one copy per key


def test_one_zero_edit_step_on_a_loader_batch(root):
    """compute_all_losses (the seam main.py calls) on a batch of the resident loader == on store.collate of the same ids, to the bit"""
    from fusions.FusionModel import FusionModel
    from fusions.load_llm import register_d_model
    from immtsf import config
    from lib.evaluation import compute_all_losses
    from models.DLinear import DLinear
    dev = _dev()
    _, res = _parsed(root, "DLinear")
    z = np.load(os.path.join(GOLDEN, "loader_DLinear.npz"))
    store, n_in, n_pred = res["ds"].store, *z["input_and_pred_len"].tolist()
    register_d_model("TOY16", 16)
    config.precision, config.nan_check = "fp32", "sync"         # (tests/conftest.py puts both back)
    a = types.SimpleNamespace(
        device=str(dev), C=store.C, enc_in=store.C, c_out=store.C, input_len=n_in, pred_len=n_pred, moving_avg=25, individual=False,
        batch_size=4, TTF_module="TTF_RecAvg", MMF_module="MMF_GR_Add", llm_model_fusion="TOY16", llm_layers_fusion=None, max_length=1024,
        use_text_embeddings=True, recency_sigma=1.0, n_heads_fusion=1, dropout=0.0, d_txt=64, kappa=0.5)
    torch.manual_seed(99)
    model, fusion = DLinear(a).to(dev).train(), FusionModel(a).to(dev).train()
    torch.manual_seed(7)
    batch = next(iter(res["train_dataloader"]))
    direct = store.collate(z["train_first.window_ids"])
    losses = []
    for b in (batch, direct):
        out = compute_all_losses(model, fusion, b, True)
        out["loss"].backward()
        losses.append(out["loss"].detach().clone())
    torch.cuda.synchronize()
    assert torch.isfinite(losses[0]) and losses[0].view(torch.int32).item() == losses[1].view(torch.int32).item(), losses
