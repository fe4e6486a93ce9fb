"""Resident dataset store + device-side batch builder.

The reference keeps the dataset as a Python list of per-window tensors and builds every batch on the host with
pad_sequence / Python loops (lib/parse_datasets.py:252-366, 764-824).  Here the whole dataset is laid out ONCE as
window-major CSR arrays in HBM (a 288 GB device holds every dataset the reference ships many times over), the
text-embedding matrices stay resident, and a batch is built by gather kernels from a list of window ids.
`collate()` returns the same dict the reference's collate returns (bit-exact) -- the standard form, tPatchGNN's patch
form, CRU's raw-time form and LatentODE's shared-axis form (:369-471) -- plus the packed ragged note index
(`note_lengths`, `note_offsets`, `note_rowmap`) that makes the zero-padded embeddings optional.

Host side (one-time, numpy): per-window metadata -- history/prediction lengths, note counts and the per-window
maximum patch population -- so output shapes are known without a device sync.  The ODE form's shapes depend on the
batch's distinct times: its axis is formed per batch from the host copy of the times (one np.unique) and sent over
with one non-blocking copy; the device is never read back.

`ResidentLoader` is the DataLoader-shaped front of the store (what lib.parse_datasets.parse_datasets returns, lib/resident_datasets.py): the epoch's whole id
order goes to the device with one copy, batch k reads its slice of it, and the standard / CRU forms are one launch per batch
(immtsf_collate_batch).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import Store, check, ptr, stream_ptr


class ResidentStore:
    def __init__(self, tt, vals, mask, row_off, note_tau, note_src, note_off, emb, history, pred_window, device):
        """numpy inputs: tt [R] f32, vals/mask [R,C] f32, row_off [W+1] i64, note_tau [S] f32, note_src [S] i64,
        note_off [W+1] i64, emb [E,d_m] f32 (the concatenated per-entity embedding matrices)."""
        self.history, self.pred_window = float(history), float(pred_window)
        self.time_max = np.float32(history + pred_window)
        self.W = len(row_off) - 1
        self.C = int(vals.shape[1])
        self.d_m = int(emb.shape[1]) if emb is not None and emb.ndim == 2 else 0
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            # "cuda" (what main.py passes) and the "cuda:0" its tensors report are different device objects: keep the resolved one
            self.device = torch.device("cuda", torch.cuda.current_device())
        # ---- host metadata
        self._tt, self._mask, self._row_off = tt, mask, row_off.astype(np.int64)
        seg = np.repeat(np.arange(self.W), np.diff(self._row_off))
        is_hist = tt < np.float32(history)
        self.hist_len = np.bincount(seg[is_hist], minlength=self.W).astype(np.int32)
        self.pred_len = (np.diff(self._row_off) - self.hist_len).astype(np.int32)
        # history rows must be a prefix of every window: times non-decreasing inside a window (the dataset sorts by time;
        # equal timestamps -- duplicate date_time rows -- are fine, the reference only splits on tt < history,
        # lib/parse_datasets.py:252-295).  One vectorised check over all rows.
        if len(tt) > 1:
            drop = np.diff(tt) < 0
            b = self._row_off[1:-1]                        # the step from one window's last row to the next window's first
            b = b[(b > 0) & (b < len(tt))]                 # (empty windows at either end have no such step)
            drop[b - 1] = False
            if np.any(drop):
                w = int(np.searchsorted(self._row_off, int(np.argmax(drop)) + 1, side="right") - 1)
                raise ValueError(f"window {w}: timestamps must be non-decreasing")
        self.n_notes = np.diff(note_off).astype(np.int32)
        self._patch_cache = {}
        # what collate() has issued so far: host-to-device copies (window ids, the ODE axis) and kernel launches
        self.h2d_copies = 0
        self.launches = 0
        # ---- device arrays
        dev = self.device
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)    # noqa: E731
        self.d = dict(tt=t(tt, np.float32), vals=t(vals, np.float32), mask=t(mask, np.float32), row_off=t(row_off, np.int64),
                      hist_len=t(self.hist_len, np.int32), note_tau=t(note_tau, np.float32), note_src=t(note_src, np.int64),
                      note_off=t(note_off, np.int64), emb=t(emb, np.float32) if self.d_m else None)
        self._struct = Store(*[None if self.d[k] is None else self.d[k].data_ptr() for k in
                               ("tt", "vals", "mask", "row_off", "hist_len", "note_tau", "note_src", "note_off", "emb")],
                             self.C, self.d_m)

    # ------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_chunks(cls, chunks, history, pred_window, device):
        """chunks: the reference dataset's list of (chunk_id, tt, vals, mask, texts) with texts = [(t, embedding)],
        exactly `ChunkedTimeSeriesDataset.chunks` (lib/parse_datasets.py:150-236).  Embedding tensors that are rows of
        one matrix (they are: `emb[i]`, :129-131) are stored once."""
        tt, vals, mask, row_off = [], [], [], [0]
        note_tau, note_src, note_off = [], [], [0]
        rows, emb_rows = {}, []
        for _, t, v, m, texts in chunks:
            tt.append(np.asarray(t, dtype=np.float32))
            vals.append(np.asarray(v, dtype=np.float32))
            mask.append(np.asarray(m, dtype=np.float32))
            row_off.append(row_off[-1] + len(tt[-1]))
            for (tn, payload) in texts:
                key = (payload.untyped_storage().data_ptr(), payload.storage_offset()) if torch.is_tensor(payload) \
                    else id(payload)
                if key not in rows:
                    rows[key] = len(emb_rows)
                    emb_rows.append(np.asarray(payload, dtype=np.float32))
                note_tau.append(np.float32(tn))
                note_src.append(rows[key])
            note_off.append(note_off[-1] + len(texts))
        emb = np.stack(emb_rows) if emb_rows else np.zeros((0, 0), np.float32)
        return cls(np.concatenate(tt), np.concatenate(vals), np.concatenate(mask), np.array(row_off, np.int64),
                   np.array(note_tau, np.float32), np.array(note_src, np.int64), np.array(note_off, np.int64), emb,
                   history, pred_window, device)

    @classmethod
    def from_dataset_dir(cls, root, history, pred_window, stride, device, time_unit="days", llm_model_fusion="GPT2",
                         llm_layers_fusion=None, max_length=1024, rec_ids=None, unit_scale=None, normalize=True, enable_text=True,
                         verbose=False):
        """Build the store from the reference's on-disk layout:
            <root>/processed/<entity>/time_series.csv                       date_time, record_id, <features...>
            <root>/processed/<entity>/text_embeddings_model={llm}_layers={n|full}_maxlen={L}.pt
                                                                            {embeddings [n,d_m] f32, rel_times [n] f32}
        and window it exactly like ChunkedTimeSeriesDataset (lib/parse_datasets.py:17-245): per-entity z-scored
        features (pandas mean / std, as there), times in `time_unit` from the entity's first observation, windows
        [st, st + history + pred_window) stepped by `stride` that hold >= 2 observations, an observed value on both
        sides of `history` and at least one note in [st, st + history).  The windows are found with searchsorted over
        the sorted times instead of a scan per window; each entity's embedding matrix goes to the device once.
        Returns (store, window_ids) with the reference's chunk ids ("<entity>_chunk<k>").

        The remaining options of ChunkedTimeSeriesDataset.__init__ (:40-77), each defaulting to what this method did without it:
        time_unit="custom" takes `unit_scale` seconds per unit; normalize=False keeps the raw features; enable_text=False is the
        unimodal run -- the embedding file is not needed, the windows are still chosen by the note times (then read from
        <entity>/text.csv, :150-170; an entity without that file yields no window) and are stored WITHOUT notes, so `tau` is (B, 0) and
        no `notes_embeddings` is emitted (:223-226); verbose=True prints the reference's per-record line (:229-233)."""
        import os
        import pandas as pd
        if time_unit == "custom":
            if unit_scale is None:
                raise ValueError("Must set unit_scale when time_unit='custom'")
            unit = float(unit_scale)
        else:
            try:
                unit = {"seconds": 1.0, "minutes": 60.0, "hours": 3600.0, "days": 86400.0, "weeks": 604800.0}[time_unit]
            except KeyError:
                raise ValueError(f"Unknown time_unit '{time_unit}'") from None
        proc = os.path.join(root, "processed")
        ents = sorted(d for d in os.listdir(proc) if os.path.isdir(os.path.join(proc, d))) if rec_ids is None else list(rec_ids)
        total = history + pred_window
        tt_all, vals_all, mask_all, row_off, ids = [], [], [], [0], []
        tau_all, src_all, note_off, embs, emb_base = [], [], [0], [], 0
        for ent in ents:
            ts_path = os.path.join(proc, ent, "time_series.csv")
            if not os.path.isfile(ts_path):
                continue
            df = pd.read_csv(ts_path)
            when = pd.to_datetime(df["date_time"])
            df = df.assign(_when=when).sort_values("_when")
            feats = [c for c in df.columns if c not in ("date_time", "record_id", "_when")]
            x = df[feats]
            if normalize:
                mu, sd = x.mean(), x.std()
                x = (x - mu) / sd.where(sd != 0, 1.0)          # z-score; constant columns are only centred
            secs = (df["_when"] - df["_when"].min()).dt.total_seconds()
            tt = (secs / unit).values.astype(np.float32)
            v32 = x.values.astype(np.float32)
            mask = (~np.isnan(v32)).astype(np.float32)
            vals = np.nan_to_num(v32, nan=0.0, posinf=np.finfo(np.float32).max, neginf=np.finfo(np.float32).min)
            if mask.sum() == 0:
                raise ValueError(f"Mask for {ent} is all zeros")
            if enable_text:
                fname = f"text_embeddings_model={llm_model_fusion}_layers={llm_layers_fusion or 'full'}_maxlen={max_length}.pt"
                path = os.path.join(proc, ent, fname)
                if not os.path.isfile(path):
                    raise FileNotFoundError(f"Missing text embeddings file: {path}")
                blob = torch.load(path, map_location="cpu")
                emb = blob["embeddings"].float().numpy()
                if np.isnan(emb).any():
                    raise ValueError("text embeddings contains NaN values.")
                rel = blob["rel_times"].float().numpy().astype(np.float64)      # what `.item()` of the fp32 times yields
                embs.append(emb)
            else:
                emb, rel = (), cls._text_csv_times(os.path.join(proc, ent, "text.csv"), df["_when"].min(), unit, ent)
            # ---- windows: st_k = t_min + k * stride while st_k + total <= t_max
            t_min, t_max = float(tt.min()), float(tt.max())
            k, cnt, dropped = 0, 0, 0
            order_ok = np.all(np.diff(tt) >= 0)
            while t_min + k * stride + total <= t_max:
                st = t_min + k * stride
                k += 1
                st32 = np.float32(st)
                if order_ok:
                    a, b = np.searchsorted(tt, st32, "left"), np.searchsorted(tt, np.float32(st + total), "left")
                    sel = np.arange(a, b)
                else:
                    sel = np.flatnonzero((tt >= st32) & (tt < np.float32(st + total)))
                if len(sel) < 2:
                    continue
                sub_tt = tt[sel] - st32
                hist = sub_tt < np.float32(history)
                if mask[sel][hist].sum() == 0 or mask[sel][~hist].sum() == 0:
                    continue
                notes = np.flatnonzero((rel >= st) & (rel < st + history))
                this = cnt
                cnt += 1
                if len(notes) == 0:          # windows without text are dropped, but they still consume a chunk number
                    dropped += 1
                    continue
                if not enable_text:
                    notes = notes[:0]        # the note times chose the window; the window itself carries no notes
                ids.append(f"{ent}_chunk{this}")
                tt_all.append(sub_tt)
                vals_all.append(vals[sel])
                mask_all.append(mask[sel])
                row_off.append(row_off[-1] + len(sel))
                tau_all.append((rel[notes] - st).astype(np.float32))
                src_all.append(notes.astype(np.int64) + emb_base)
                note_off.append(note_off[-1] + len(notes))
            emb_base += len(emb)
            if verbose:      # the reference counts a dropped window in both numbers (its cnt moves before the drop)
                print(f"Record {ent}: {cnt} chunks created, {dropped} dropped ({dropped / max(cnt + dropped, 1):.2%})")
        if not ids:
            raise RuntimeError("No chunks created; check history/pred_window/stride")
        if not enable_text:     # no notes anywhere: one unreferenced entry keeps the two note arrays' device pointers non-null
            tau_all, src_all, embs = [np.zeros(1, np.float32)], [np.zeros(1, np.int64)], [np.zeros((0, 0), np.float32)]
        store = cls(np.concatenate(tt_all), np.concatenate(vals_all), np.concatenate(mask_all), np.array(row_off, np.int64),
                    np.concatenate(tau_all), np.concatenate(src_all), np.array(note_off, np.int64), np.concatenate(embs),
                    history, pred_window, device)
        return store, ids

    @staticmethod
    def _text_csv_times(path, base, unit, ent):
        """the note times of <entity>/text.csv in dataset units from the entity's first observation, as float64 (the reference's
        raw-text branch, lib/parse_datasets.py:150-170): rows sorted by date, exactly one text column, empty notes skipped"""
        import os
        import pandas as pd
        if not os.path.isfile(path):
            return np.zeros(0, np.float64)
        tdf = pd.read_csv(path, parse_dates=["date_time"]).sort_values("date_time")
        cols = [c for c in tdf.columns if c not in ("date_time", "record_id")]
        if len(cols) != 1:
            raise ValueError(f"{ent}: expected 1 text column, got {cols}")
        tdf = tdf[~tdf[cols[0]].isna()]
        return ((tdf["date_time"] - base).dt.total_seconds() / unit).values.astype(np.float64)

    # ------------------------------------------------------------------------------------------ batches
    def _ids(self, window_ids, ids_dev=None):
        """-> (host ids, device ids).  ids_dev: the same ids already on the device (int32, contiguous -- ResidentLoader's slice of its
        epoch order), in which case nothing is copied; the host ids still size every output."""
        ids = np.asarray(window_ids, dtype=np.int32)
        if ids.ndim != 1 or (len(ids) and (ids.min() < 0 or ids.max() >= self.W)):
            raise IndexError("window ids out of range")
        if ids_dev is not None:
            if ids_dev.dtype != torch.int32 or ids_dev.shape != (len(ids),) or not ids_dev.is_contiguous() or ids_dev.device != self.device:
                raise ValueError("device ids must be a contiguous int32 vector on the store's device, as long as the host ids")
            return ids, ids_dev
        self.h2d_copies += 1
        return ids, torch.from_numpy(ids).to(self.device, non_blocking=True)

    def _patch_max(self, patch_size, npatch, patch_stride):
        """per window: max over (patch, variable) of the number of observed history points -- one kernel over the resident arrays,
        W int32 copied to the host once per key"""
        key = (patch_size, npatch, patch_stride)
        if key not in self._patch_cache:
            out = torch.empty(self.W, dtype=torch.int32, device=self.device)
            check(_lib.load().immtsf_collate_patch_max(C.byref(self._struct), self.W, npatch, float(patch_size), float(patch_stride),
                                                       self.history, ptr(out), stream_ptr()), "collate_patch_max")
            self._patch_cache[key] = out.cpu().numpy()
        return self._patch_cache[key]

    def _patch_max_host(self, patch_size, npatch, patch_stride):
        """_patch_max as a loop over every window x patch on the host copy: the reference the kernel is tested against"""
        out = np.zeros(self.W, dtype=np.int32)
        for w in range(self.W):
            a = self._row_off[w]
            t, m = self._tt[a:a + self.hist_len[w]], self._mask[a:a + self.hist_len[w]]
            for i in range(npatch):
                st = np.float32(i * patch_stride)
                ed = np.float32(self.history if i == npatch - 1 else i * patch_stride + patch_size)
                sel = (t >= st) & (t < ed)
                if sel.any():
                    out[w] = max(out[w], int((m[sel] != 0).sum(0).max()))
        return out

    def _union_axis(self, ids):
        """-> (axis, n_obs): the sorted distinct fp32 times over all rows of the batch's windows and how many lie below `history`
        (what torch.unique / torch.lt give the reference, lib/parse_datasets.py:418-424).  Host only: one sort of the batch's rows."""
        ro = self._row_off
        axis = np.unique(np.concatenate([self._tt[ro[w]:ro[w + 1]] for w in ids])) if len(ids) else np.zeros(0, np.float32)
        return axis, int(np.searchsorted(axis, np.float32(self.history), side="left"))

    def collate(self, window_ids, patch=None, padded_notes=True, form="standard", _ids_dev=None, _one_launch=False):
        """-> dict of device tensors.  patch=None: the standard collate's keys; patch=(patch_size, npatch, patch_stride):
        tPatchGNN's.  form="cru": the standard keys with the stored chunk-relative times (not normalised); form="ode": LatentODE's
        -- one shared time axis, observed_tp (n_obs,) / tp_to_predict (T - n_obs,) and (B, n_obs | T - n_obs, C) grids.
        Always: tau, note_lengths, note_offsets, note_rowmap (+ notes_embeddings unless padded_notes=False).
        Internal (ResidentLoader): _ids_dev = the ids already on the device (no copy here); _one_launch = build a standard / CRU batch
        with immtsf_collate_batch instead of the series + note kernels -- the same tensors."""
        if form not in ("standard", "cru", "ode"):
            raise ValueError(f"unknown collate form {form!r}: 'standard', 'cru' or 'ode'")
        if patch is not None and form != "standard":
            raise ValueError(f"patch= builds tPatchGNN's form; it cannot be combined with form={form!r}")
        lib = _lib.load()
        ids, ids_dev = self._ids(window_ids, _ids_dev)
        B, dev, f32 = len(ids), self.device, torch.float32
        if _one_launch and B and patch is None and form != "ode":
            return self._collate_batch(lib, ids, ids_dev, padded_notes, 1.0 if form == "cru" else float(self.time_max))
        if form == "ode":
            out = self._collate_union(lib, ids, ids_dev)
            if B:
                self._collate_notes(lib, out, ids, ids_dev, padded_notes)
            else:
                self._empty_notes(out, padded_notes)
            return out
        Lmax = int(self.hist_len[ids].max()) if B else 0
        Lpmax = int(self.pred_len[ids].max()) if B else 0
        out = {"tp_to_predict": torch.empty(B, Lpmax, dtype=f32, device=dev),
               "data_to_predict": torch.empty(B, Lpmax, self.C, dtype=f32, device=dev),
               "mask_predicted_data": torch.empty(B, Lpmax, self.C, dtype=f32, device=dev)}
        st = C.byref(self._struct)
        if B == 0:          # nothing to launch (empty tensors have no device pointer)
            shp = (0, 0, self.C) if patch is None else (0, patch[1], 0, self.C)
            out.update(observed_tp=torch.empty(shp[:-1], dtype=f32, device=dev), observed_data=torch.empty(shp, dtype=f32, device=dev),
                       observed_mask=torch.empty(shp, dtype=f32, device=dev))
            self._empty_notes(out, padded_notes)
            return out
        if patch is None:
            out.update(observed_tp=torch.empty(B, Lmax, dtype=f32, device=dev),
                       observed_data=torch.empty(B, Lmax, self.C, dtype=f32, device=dev),
                       observed_mask=torch.empty(B, Lmax, self.C, dtype=f32, device=dev))
            # CRU's collate (lib/parse_datasets.py:369-408) is the standard one without the time normalisation.  The kernel computes
            # (t - 0) / scale with scale = time_max + (time_max == 0) * 1e-8; at time_max = 1 that is t / 1, which IEEE division
            # returns as t bit for bit (and the padding stays 0), so the raw-time form needs no kernel of its own.
            time_max = 1.0 if form == "cru" else float(self.time_max)
            check(lib.immtsf_collate_series(st, ptr(ids_dev), B, Lmax, Lpmax, time_max, ptr(out["observed_tp"]),
                                            ptr(out["observed_data"]), ptr(out["observed_mask"]), ptr(out["tp_to_predict"]),
                                            ptr(out["data_to_predict"]), ptr(out["mask_predicted_data"]), stream_ptr()),
                  "collate_series")
            self.launches += 1
        else:
            ps, npatch, pstride = patch
            Lp = int(self._patch_max(ps, npatch, pstride)[ids].max()) if B else 0
            for k in ("observed_tp", "observed_data", "observed_mask"):
                out[k] = torch.empty(B, npatch, Lp, self.C, dtype=f32, device=dev)
            check(lib.immtsf_collate_series(st, ptr(ids_dev), B, 0, Lpmax, float(self.time_max), None, None, None,
                                            ptr(out["tp_to_predict"]), ptr(out["data_to_predict"]),
                                            ptr(out["mask_predicted_data"]), stream_ptr()), "collate_series")
            check(lib.immtsf_collate_patches(st, ptr(ids_dev), B, npatch, float(ps), float(pstride), self.history, Lp,
                                             float(self.time_max), ptr(out["observed_tp"]), ptr(out["observed_data"]),
                                             ptr(out["observed_mask"]), stream_ptr()), "collate_patches")
            self.launches += 2 if Lp else 1
        self._collate_notes(lib, out, ids, ids_dev, padded_notes)
        return out

    def _collate_batch(self, lib, ids, ids_dev, padded_notes, time_max):
        """a standard (time_max = history + pred_window) or CRU (time_max = 1, see collate) batch of B >= 1 windows: one launch"""
        B, dev, f32, i32 = len(ids), self.device, torch.float32, torch.int32
        Lmax, Lpmax = int(self.hist_len[ids].max()), int(self.pred_len[ids].max())
        Nmax, total = int(self.n_notes[ids].max()), int(self.n_notes[ids].sum())
        out = {"tp_to_predict": torch.empty(B, Lpmax, dtype=f32, device=dev),
               "data_to_predict": torch.empty(B, Lpmax, self.C, dtype=f32, device=dev),
               "mask_predicted_data": torch.empty(B, Lpmax, self.C, dtype=f32, device=dev),
               "observed_tp": torch.empty(B, Lmax, dtype=f32, device=dev),
               "observed_data": torch.empty(B, Lmax, self.C, dtype=f32, device=dev),
               "observed_mask": torch.empty(B, Lmax, self.C, dtype=f32, device=dev),
               "tau": torch.empty(B, Nmax, dtype=f32, device=dev),
               "note_lengths": torch.empty(B, dtype=i32, device=dev),
               "note_offsets": torch.empty(B + 1, dtype=i32, device=dev),
               "note_rowmap": torch.empty(total, dtype=i32, device=dev)}
        notes = None
        if padded_notes and self.d_m:
            notes = out["notes_embeddings"] = torch.empty(B, Nmax, self.d_m, dtype=f32, device=dev)
        check(lib.immtsf_collate_batch(C.byref(self._struct), ptr(ids_dev), B, Lmax, Lpmax, Nmax, time_max, ptr(out["observed_tp"]),
                                       ptr(out["observed_data"]), ptr(out["observed_mask"]), ptr(out["tp_to_predict"]),
                                       ptr(out["data_to_predict"]), ptr(out["mask_predicted_data"]), ptr(out["tau"]), ptr(notes),
                                       ptr(out["note_lengths"]), ptr(out["note_offsets"]), ptr(out["note_rowmap"]), stream_ptr()),
              "collate_batch")
        self.launches += 1
        if self.d_m:
            from .ops import PackedNotes
            out["notes_packed"] = PackedNotes(self.d["emb"], out["note_rowmap"], out["note_lengths"], Nmax)
        return out

    def _collate_union(self, lib, ids, ids_dev):
        """the six keys of form="ode" (variable_time_collate_fn_ODE, lib/parse_datasets.py:411-471): one launch"""
        B, dev, f32 = len(ids), self.device, torch.float32
        axis, n_obs = self._union_axis(ids)
        T = len(axis)
        out = {"observed_tp": torch.empty(n_obs, dtype=f32, device=dev),
               "observed_data": torch.empty(B, n_obs, self.C, dtype=f32, device=dev),
               "observed_mask": torch.empty(B, n_obs, self.C, dtype=f32, device=dev),
               "tp_to_predict": torch.empty(T - n_obs, dtype=f32, device=dev),
               "data_to_predict": torch.empty(B, T - n_obs, self.C, dtype=f32, device=dev),
               "mask_predicted_data": torch.empty(B, T - n_obs, self.C, dtype=f32, device=dev)}
        if B == 0 or T == 0:          # nothing to launch
            return out
        # the axis goes over from pinned memory without blocking; the caching host allocator keeps the block until the copy has run
        staged = torch.empty(T, dtype=f32, pin_memory=True)
        staged.numpy()[:] = axis
        axis_dev = staged.to(dev, non_blocking=True)
        self.h2d_copies += 1
        check(lib.immtsf_collate_union(C.byref(self._struct), ptr(ids_dev), B, ptr(axis_dev), T, n_obs, float(self.time_max),
                                       ptr(out["observed_tp"]), ptr(out["observed_data"]), ptr(out["observed_mask"]),
                                       ptr(out["tp_to_predict"]), ptr(out["data_to_predict"]), ptr(out["mask_predicted_data"]),
                                       stream_ptr()), "collate_union")
        self.launches += 1
        return out

    def _empty_notes(self, out, padded_notes):
        """the multimodal part of a batch of no windows"""
        dev = self.device
        out.update(tau=torch.empty(0, 0, dtype=torch.float32, device=dev), note_lengths=torch.empty(0, dtype=torch.int32, device=dev),
                   note_offsets=torch.zeros(1, dtype=torch.int32, device=dev), note_rowmap=torch.empty(0, dtype=torch.int32, device=dev))
        if padded_notes and self.d_m:
            out["notes_embeddings"] = torch.empty(0, 0, self.d_m, dtype=torch.float32, device=dev)

    def _collate_notes(self, lib, out, ids, ids_dev, padded_notes):
        """the multimodal part, the same for every form: tau, the padded embeddings and the packed ragged note index"""
        B, dev, f32 = len(ids), self.device, torch.float32
        st = C.byref(self._struct)
        Nmax = int(self.n_notes[ids].max()) if B else 0
        total = int(self.n_notes[ids].sum()) if B else 0
        out["tau"] = torch.empty(B, Nmax, dtype=f32, device=dev)
        out["note_lengths"] = torch.empty(B, dtype=torch.int32, device=dev)
        out["note_offsets"] = torch.empty(B + 1, dtype=torch.int32, device=dev)
        out["note_rowmap"] = torch.empty(total, dtype=torch.int32, device=dev)
        notes = None
        if padded_notes and self.d_m:
            notes = out["notes_embeddings"] = torch.empty(B, Nmax, self.d_m, dtype=f32, device=dev)
        check(lib.immtsf_collate_notes(st, ptr(ids_dev), B, Nmax, ptr(out["tau"]), ptr(notes), ptr(out["note_lengths"]),
                                       ptr(out["note_offsets"]), ptr(out["note_rowmap"]), stream_ptr()), "collate_notes")
        self.launches += 2 if B and Nmax else 1
        if self.d_m:
            from .ops import PackedNotes
            out["notes_packed"] = PackedNotes(self.d["emb"], out["note_rowmap"], out["note_lengths"], Nmax)


class _Windows:
    """what `loader.dataset` is asked for: a length"""

    def __init__(self, n):
        self._n = int(n)

    def __len__(self):
        return self._n


class ResidentLoader:
    """A DataLoader-shaped iterable over some windows of a ResidentStore: each item is `store.collate(ids, ...)` of the next
    `batch_size` windows (the last batch is partial), built on the caller's current stream into fresh tensors.

    Order: `window_ids` as given, or (shuffle=True) the order `DataLoader(Subset(ds, window_ids), batch_size, shuffle=True)` visits --
    torch's own RandomSampler / BatchSampler over range(len(window_ids)) and the base-seed draw a DataLoader makes when it is
    iterated, so the global RNG (or `generator`) is left exactly where a DataLoader leaves it.  At `__iter__` the epoch's whole order
    goes to the device with ONE non-blocking copy; batch k hands collate() its slice, so no batch uploads ids (the ODE form still
    uploads its time axis: that is data).  form "standard" / "cru" without `patch` is one launch per batch (immtsf_collate_batch).
    `h2d_copies` counts the host-to-device copies issued so far, `launches` the kernel launches."""

    def __init__(self, store, window_ids, batch_size, shuffle, form="standard", patch=None, padded_notes=True, generator=None):
        if form not in ("standard", "cru", "ode"):
            raise ValueError(f"unknown collate form {form!r}: 'standard', 'cru' or 'ode'")
        if patch is not None and form != "standard":
            raise ValueError(f"patch= builds tPatchGNN's form; it cannot be combined with form={form!r}")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be a positive integer")
        self.store, self.batch_size, self.shuffle = store, int(batch_size), bool(shuffle)
        self.form, self.patch, self.padded_notes, self.generator = form, None if patch is None else tuple(patch), padded_notes, generator
        self.window_ids = np.asarray(window_ids, dtype=np.int32).reshape(-1)
        if len(self.window_ids) and (self.window_ids.min() < 0 or self.window_ids.max() >= store.W):
            raise IndexError("window ids out of range")
        self.dataset = _Windows(len(self.window_ids))
        self.h2d_copies = 0
        self.launches = 0

    def __len__(self):
        return -(-len(self.window_ids) // self.batch_size)

    def _epoch_order(self):
        """positions into window_ids in the order this epoch visits them (host only; draws what a DataLoader draws)"""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        n = len(self.window_ids)
        sampler = RandomSampler(range(n), generator=self.generator) if self.shuffle else SequentialSampler(range(n))
        batches = iter(BatchSampler(sampler, self.batch_size, drop_last=False))
        # a DataLoader draws its per-iterator base seed here, shuffling or not, before the sampler draws anything
        torch.empty((), dtype=torch.int64).random_(generator=self.generator)
        return np.fromiter((i for batch in batches for i in batch), dtype=np.int64, count=n)

    def __iter__(self):
        """the RNG draws and the upload of the epoch's ids happen here, as a DataLoader's do at iter(); the batches are built lazily"""
        order = self.window_ids[self._epoch_order()]
        n, st = len(order), self.store
        if n == 0:
            return iter(())
        # pinned, so the copy does not block; the caching host allocator keeps the block until the copy has run
        staged = torch.empty(n, dtype=torch.int32, pin_memory=True)
        staged.numpy()[:] = order
        ids_dev = staged.to(st.device, non_blocking=True)
        self.h2d_copies += 1
        return self._batches(order, ids_dev)

    def _batches(self, order, ids_dev):
        n, bs, st = len(order), self.batch_size, self.store
        one = self.patch is None and self.form != "ode"
        for k in range(0, n, bs):
            c0, l0 = st.h2d_copies, st.launches
            batch = st.collate(order[k:k + bs], patch=self.patch, padded_notes=self.padded_notes, form=self.form,
                               _ids_dev=ids_dev[k:k + bs], _one_launch=one)
            self.h2d_copies += st.h2d_copies - c0
            self.launches += st.launches - l0
            yield batch
