"""Loaders -- counterpart of src/dataloaders.py:8-59 (same function names, arguments and defaults).

`make_loader` / `create_dataloaders` return ordinary torch DataLoaders over `AudioDeepfakeDataset`, so reference
scripts keep working.  `FlatBatcher` is the ingest path sized for the GPU: one contiguous (optionally pinned) tensor,
batches are slices, host->device copies are asynchronous on a side stream and double-buffered.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import dataset as ds


def create_dataloaders(train_features_path, train_labels_path, dev_features_path, dev_labels_path,
                       test_features_path, batch_size=32, num_workers=2):
    """(train_loader [shuffled], dev_loader, test_loader [features only]) -- src/dataloaders.py:8-52."""
    train = ds.AudioDeepfakeDataset(train_features_path, train_labels_path)
    dev = ds.AudioDeepfakeDataset(dev_features_path, dev_labels_path)
    test = ds.AudioDeepfakeDataset(test_features_path, None)
    kw = dict(batch_size=batch_size, num_workers=num_workers, pin_memory=True)
    return (DataLoader(train, shuffle=True, **kw), DataLoader(dev, shuffle=False, **kw),
            DataLoader(test, shuffle=False, **kw))


def make_loader(features_path, labels_path, batch_size=32, num_workers=2, shuffle=False):
    """src/dataloaders.py:55-59."""
    return DataLoader(ds.AudioDeepfakeDataset(features_path, labels_path), batch_size=batch_size, shuffle=shuffle,
                      num_workers=num_workers)


def train_shard_indices(perm: torch.Tensor, batch_size: int, rank: int = 0, world: int = 1) -> torch.Tensor:
    """Sample indices of `rank` for one data-parallel training epoch over the permutation `perm`.

    Global batch g is perm[g*world*bs : (g+1)*world*bs]; rank r takes rows [r*bs, (r+1)*bs) of it.  With world > 1 the
    permutation is padded by wrap-around to a multiple of world*bs (DistributedSampler semantics), so EVERY rank runs
    the same number of steps with the same local batch size: one all-reduce per step on every rank (no hang on a short
    last shard) and the 1/world gradient scale is exact.  world == 1 keeps the reference's ragged last batch
    (src/train.py:61: the DataLoader's final short batch)."""
    n = perm.numel()
    if world <= 1 or n == 0:
        return perm
    gb = world * batch_size
    total = -(-n // gb) * gb
    reps = -(-total // n)
    ext = perm.repeat(reps)[:total] if reps > 1 else perm
    return ext.view(-1, world, batch_size)[:, rank].reshape(-1)


class FlatBatcher:
    """Iterate (features [b,180,321] on `device`, labels [b] on `device` or None) over a stacked dataset.

    rank/world shard the utterance range contiguously (rank r gets [r*ceil(N/world), ...)): the data-parallel
    inference partition of SURVEY.md section 8(e); order inside a shard is preserved so host code can concatenate.
    """

    def __init__(self, features: torch.Tensor, labels: torch.Tensor | None, batch_size: int, device="cuda",
                 rank: int = 0, world: int = 1, dtype: torch.dtype | None = None):
        n = features.shape[0]
        per = -(-n // world)
        self.lo, self.hi = min(rank * per, n), min((rank + 1) * per, n)
        self.features, self.labels = features, labels
        self.batch_size, self.device, self.dtype = batch_size, torch.device(device), dtype
        self._registered = None

    def __len__(self):
        return -(-(self.hi - self.lo) // self.batch_size)

    # A pageable source (the memory-mapped flat file) makes every H2D copy block the host for its duration, so the next forward
    # is launched only after the next batch's copy has finished (measured 0.85 ms per 256-utterance batch for 0.67 ms of kernels).
    # Registering this rank's share of the mapping with the HIP runtime (hipHostRegister: the pages are pinned where they are, no
    # staging copy) makes the copies asynchronous; above `max_register_bytes` (or if the runtime refuses) the pageable path stays.
    max_register_bytes = 16 << 30

    def _register(self):
        f = self.features
        if self._registered is not None or self.device.type != "cuda" or f.device.type != "cpu" or f.is_pinned() or self.hi <= self.lo:
            return
        try:
            if not f[self.lo:self.hi].is_contiguous():
                return
            ptr = f[self.lo:self.hi].data_ptr()
            nbytes = (self.hi - self.lo) * f[0].numel() * f.element_size()
            if nbytes > self.max_register_bytes:
                return
            if int(torch.cuda.cudart().cudaHostRegister(ptr, nbytes, 0)) == 0:
                self._registered = ptr
        except Exception:   # noqa: BLE001 -- an optimisation only
            self._registered = None

    def _unregister(self):
        if self._registered is not None:
            try:
                torch.cuda.synchronize(self.device)
                torch.cuda.cudart().cudaHostUnregister(self._registered)
            except Exception:   # noqa: BLE001
                pass
            self._registered = None

    def __del__(self):
        self._unregister()

    def _put(self, lo, hi, stream):
        with torch.cuda.stream(stream):
            f = self.features[lo:hi].to(self.device, non_blocking=True)
            if self.dtype is not None:
                f = f.to(self.dtype)
            l = None if self.labels is None else self.labels[lo:hi].to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        return f, l, ev

    def __iter__(self):
        if self.device.type != "cuda":
            for lo in range(self.lo, self.hi, self.batch_size):
                hi = min(lo + self.batch_size, self.hi)
                yield self.features[lo:hi], (None if self.labels is None else self.labels[lo:hi])
            return
        self._register()
        copy_stream = torch.cuda.Stream(self.device)
        starts = list(range(self.lo, self.hi, self.batch_size))
        nxt = self._put(starts[0], min(starts[0] + self.batch_size, self.hi), copy_stream) if starts else None
        try:
            for i, lo in enumerate(starts):
                f, l, ev = nxt
                if i + 1 < len(starts):
                    nlo = starts[i + 1]
                    nxt = self._put(nlo, min(nlo + self.batch_size, self.hi), copy_stream)
                torch.cuda.current_stream(self.device).wait_event(ev)
                f.record_stream(torch.cuda.current_stream(self.device))
                if l is not None:
                    l.record_stream(torch.cuda.current_stream(self.device))
                yield f, l
        finally:
            self._unregister()

    def restore(self, outputs):
        """Per-batch outputs -> one tensor in input order (the batches already are)."""
        return torch.cat(list(outputs))


class IndexedFlatBatcher:
    """Batches of ARBITRARY rows of a flat [N,180,321] source -- the data-parallel TRAINING loader (the
    reference's shuffled DataLoader, src/dataloaders.py:55-59 / src/train.py:279-285, on every rank's share).

    `features` is any row-indexable tensor: the zero-copy view of a memory-mapped flat file (ingest.FlatFeatures.tensor(): a
    rank then reads ONLY the rows it trains on -- 1/world of the set per epoch, never the whole pickle) or an in-memory stack.
    `indices` are this rank's sample indices for the epoch in consumption order (dataloaders.train_shard_indices).  Each batch is
    gathered on the host into a (pinned) staging buffer and copied to the device on a side stream, one batch ahead of the
    consumer.  `rows_fetched` / `bytes_fetched` count what this rank pulled from the source."""

    def __init__(self, features: torch.Tensor, labels: torch.Tensor | None, indices: torch.Tensor, batch_size: int,
                 device="cuda", dtype: torch.dtype | None = None, pin: bool = True):
        self.features, self.labels = features, labels
        self.indices = indices.to(torch.int64).reshape(-1)
        self.batch_size, self.device, self.dtype = int(batch_size), torch.device(device), dtype
        self.pin = bool(pin) and self.device.type == "cuda"
        self.rows_fetched = 0
        self.bytes_fetched = 0
        self._row_bytes = int(features[0].numel() * features.element_size()) if len(features) else 0
        self._stage, self._stage_ev = [None, None], [None, None]      # two persistent (pinned) staging buffers + their last H2D events
        self._pool = None

    copy_threads = 4          # worker threads of the row gather (plain memcpys; 1 = on the calling thread)

    def __len__(self):
        return -(-self.indices.numel() // self.batch_size)

    def _gather(self, lo, hi, slot=None):
        """Rows indices[lo:hi] of the source.  slot = None: a fresh tensor (CPU consumers); slot = k: copied row by row into the
        k-th of two persistent pinned staging buffers -- `features[idx]` allocates (and page-faults) a new 59 MB tensor per fp32
        batch and `pin_memory()` copies it again: 50 ms per 256 utterances on the GPU box, ten training steps' worth; 256 plain
        231 KB row copies into a buffer that already exists take 2.8 ms (tools/gpu_loader_probe2.py)."""
        idx = self.indices[lo:hi]
        n = int(idx.numel())
        self.rows_fetched += n
        self.bytes_fetched += n * self._row_bytes
        lab = None if self.labels is None else self.labels[idx]
        if slot is None:
            return self.features[idx], lab              # fancy index: copies exactly these rows out of the (memory-mapped) source
        if self._stage[slot] is None:
            buf = torch.empty((self.batch_size, *self.features.shape[1:]), dtype=self.features.dtype)
            self._stage[slot] = buf.pin_memory() if self.pin else buf
        if self._stage_ev[slot] is not None:
            self._stage_ev[slot].synchronize()           # the H2D copy that last read this buffer has finished (long ago)
        rows = self._stage[slot][:n]
        # one plain memcpy per row on this thread (ctypes.memmove): torch's copy / index kernels fan a 231 KB row out over every
        # CPU the machine REPORTS (128 on the GPU box, 16 of them ours: 112 ms per batch), numpy.take buffers (14 ms)
        import ctypes
        src, dst, rb = self.features.data_ptr(), rows.data_ptr(), self._row_bytes
        if self.features.is_contiguous():
            rl = idx.tolist()

            def copy_rows(j0, j1):                      # (ctypes releases the GIL inside memmove: the chunks run in parallel)
                for j in range(j0, j1):
                    ctypes.memmove(dst + j * rb, src + rl[j] * rb, rb)
            nw = self.copy_threads if n >= 4 * self.copy_threads else 1
            if nw > 1:
                if self._pool is None:
                    from concurrent.futures import ThreadPoolExecutor
                    self._pool = ThreadPoolExecutor(max_workers=nw)
                step = -(-n // nw)
                list(self._pool.map(lambda k: copy_rows(k * step, min(n, (k + 1) * step)), range(nw)))
            else:
                copy_rows(0, n)
        else:
            for j, r in enumerate(idx.tolist()):
                rows[j].copy_(self.features[r])
        return rows, lab

    def _put(self, lo, hi, stream, slot=0):
        rows, lab = self._gather(lo, hi, slot)
        with torch.cuda.stream(stream):
            f = rows.to(self.device, non_blocking=True)
            if self.dtype is not None:
                f = f.to(self.dtype)
            l = None if lab is None else lab.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._stage_ev[slot] = ev
        return f, l, ev, rows                           # `rows` keeps the pinned staging buffer alive until the copy is consumed

    def __iter__(self):
        n = self.indices.numel()
        starts = list(range(0, n, self.batch_size))
        if self.device.type != "cuda":
            for lo in starts:
                rows, lab = self._gather(lo, min(lo + self.batch_size, n))
                yield (rows if self.dtype is None else rows.to(self.dtype)), lab
            return
        copy_stream = torch.cuda.Stream(self.device)
        nxt = self._put(starts[0], min(starts[0] + self.batch_size, n), copy_stream, 0) if starts else None
        for i, lo in enumerate(starts):
            f, l, ev, _keep = nxt
            if i + 1 < len(starts):
                nlo = starts[i + 1]
                nxt = self._put(nlo, min(nlo + self.batch_size, n), copy_stream, (i + 1) & 1)
            torch.cuda.current_stream(self.device).wait_event(ev)
            f.record_stream(torch.cuda.current_stream(self.device))
            if l is not None:
                l.record_stream(torch.cuda.current_stream(self.device))
            yield f, l


class ResidentBatcher:
    """The training set held in HBM: the flat [N,180,321] source is uploaded ONCE (in chunks, optionally rounded to bf16 on the
    device) and a batch is a row gather on the device (`index_select`: 59 MB in ~40 us).  An MI355X has 288 GB: 100 k utterances
    are 23 GB in fp32, so for the reference's data sets the host never takes part in an epoch again -- the loop runs at the speed
    of the training step (the host-fed IndexedFlatBatcher delivers ~100 k utterances/s per rank; the CNN1D step consumes 430 k).
    Same interface and batch contents as IndexedFlatBatcher(features, labels, indices, batch_size): `epoch(indices)` returns the
    iterable for one epoch's index order (dataloaders.train_shard_indices).
    norm: "cmn" / "cvmn" normalise every stored utterance [180, 321] over its frames (normalization.normalize_batch) as its
    chunk arrives, in float32 and before any rounding to bf16: once per set, nothing per epoch."""

    def __init__(self, features: torch.Tensor, labels: torch.Tensor | None, batch_size: int, device="cuda",
                 dtype: torch.dtype | None = None, chunk_rows: int = 2048, norm: str = "raw"):
        from .normalization import check_mode, normalize_batch
        self.device, self.batch_size, self.norm = torch.device(device), int(batch_size), check_mode(norm)
        n = features.shape[0]
        store = dtype or features.dtype
        self.features = torch.empty((n, *features.shape[1:]), dtype=store, device=self.device)
        for lo in range(0, n, chunk_rows):                   # bounded host staging: the source is a memory map
            hi = min(n, lo + chunk_rows)
            chunk = features[lo:hi].to(self.device, non_blocking=False)
            if norm != "raw":                                # the stored [n, F, T] chunk as the [n, T, F] batch the call takes
                chunk = normalize_batch(chunk.float().transpose(1, 2), norm).transpose(1, 2)
            self.features[lo:hi].copy_(chunk)
        self.labels = None if labels is None else labels.to(self.device)
        self.bytes_resident = self.features.numel() * self.features.element_size()

    @staticmethod
    def fits(features: torch.Tensor, device, dtype: torch.dtype | None = None, fraction: float = 0.5) -> bool:
        """True when the whole set takes at most `fraction` of the device's currently free memory."""
        dev = torch.device(device)
        if dev.type != "cuda":
            return False
        es = torch.empty((), dtype=dtype or features.dtype).element_size()
        free, _total = torch.cuda.mem_get_info(dev)
        return features.numel() * es <= fraction * free

    def epoch(self, indices: torch.Tensor):
        idx = indices.to(self.device, dtype=torch.int64).reshape(-1)
        bs, feats, labels = self.batch_size, self.features, self.labels

        class _Epoch:
            def __len__(self_inner):
                return -(-idx.numel() // bs)

            def __iter__(self_inner):
                for lo in range(0, idx.numel(), bs):
                    rows = idx[lo:lo + bs]
                    yield feats.index_select(0, rows), (None if labels is None else labels.index_select(0, rows))
        return _Epoch()


def plan_packed_set(lengths, C: int):
    """(offsets int64[N], total_floats) of a packed set of N utterances [C, T_i], time fastest: utterance i is C rows of
    pitch_i = ceil(T_i / 4) * 4 floats from float offset offsets[i], back to back in input order.  Every offset is a multiple of
    4, so on a 16-byte aligned base every row starts on 16 bytes.  Pure host arithmetic in int64 (a set may exceed 2^31 floats)."""
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if int(C) < 1 or (lens.size and int(lens.min()) < 1):
        raise ValueError("a packed set needs C >= 1 and every length >= 1")
    sizes = int(C) * ((lens + 3) // 4 * 4)
    ends = np.cumsum(sizes, dtype=np.int64)
    offsets = np.zeros(lens.size, dtype=np.int64)
    offsets[1:] = ends[:-1]
    return offsets, (int(ends[-1]) if lens.size else 0)


class DlqResidentSet:
    """A DeepfakeDetector training or dev set held in HBM: the per-utterance [C, T_i] tensors of a
    features.pkl are uploaded ONCE, packed (plan_packed_set), and `batch(idx, spans)` assembles the padded, optionally
    SpecAugmented batch of any utterances with one HIP launch (dfa_dlq_gather_batch) in the layout DlqTrainer.step and the eval
    forward read in place.  Per batch the host sends the table alone: offsets, lengths and mask spans, a few hundred bytes.
    What ResidentBatcher is to the equal-length models; utterances of unequal lengths and per-sample masks need a kernel.

    offsets / lengths: host numpy arrays (int64 / int32); labels: float32 device tensor, labels_host its numpy copy (or None);
    set: the packed float32 device buffer (the floats T_i .. pitch_i of a row are unspecified); bytes_resident.
    norm: "cmn" / "cvmn" normalise every utterance of the set in place, once, after the upload (dfa_utt_norm_packed): the gather's
    SpecAugment spans then mask normalised data, the reference's order (its dataset normalises, its training loop masks)."""

    def __init__(self, feature_list, labels=None, device="cuda", chunk_utts: int = 1024, norm: str = "raw"):
        from . import _lib
        from .normalization import check_mode, normalize_packed_
        self.norm = check_mode(norm)
        self.device = torch.device(device)
        self.ctx = _lib.Context.get(self.device)               # (raises off the GPU: there is no CPU path)
        if len(feature_list) == 0:
            raise ValueError("DlqResidentSet needs at least one utterance")
        chans = {int(f.shape[0]) for f in feature_list}
        if len(chans) != 1:
            raise ValueError(f"utterances must share the feature dimension, got {sorted(chans)}")
        self.C = chans.pop()
        self.lengths = np.array([int(f.shape[-1]) for f in feature_list], dtype=np.int32)
        self.offsets, self.total_floats = plan_packed_set(self.lengths, self.C)
        dev = torch.device("cuda", self.ctx.index)
        self.set = torch.empty(self.total_floats, dtype=torch.float32, device=dev)
        if self.set.data_ptr() % 256:
            raise RuntimeError("the resident buffer is not 256-byte aligned")
        n = len(feature_list)
        ends = np.append(self.offsets[1:], self.total_floats)
        for lo in range(0, n, max(1, int(chunk_utts))):          # bounded host staging, as ResidentBatcher's
            hi = min(n, lo + max(1, int(chunk_utts)))
            base = int(self.offsets[lo])
            host = torch.zeros(int(ends[hi - 1]) - base, dtype=torch.float32)
            for i in range(lo, hi):
                T = int(self.lengths[i])
                rows = host[int(self.offsets[i]) - base:int(ends[i]) - base].view(self.C, -1)
                rows[:, :T] = torch.as_tensor(feature_list[i]).float()
            self.set[base:int(ends[hi - 1])].copy_(host)
        with torch.cuda.device(self.ctx.index):
            normalize_packed_(self.set, self.offsets, self.lengths, self.C, norm)
        self.labels_host = None if labels is None else np.asarray(labels, dtype=np.float32).reshape(-1)
        if self.labels_host is not None and self.labels_host.shape[0] != n:
            raise ValueError(f"got {self.labels_host.shape[0]} labels for {n} utterances")
        self.labels = None if labels is None else torch.from_numpy(self.labels_host.copy()).to(dev)
        self.bytes_resident = self.set.numel() * 4
        self._x = None          # the batch buffer, grown when needed and reused from batch to batch
        self._tab = None        # the kernel's per-call table

    def __len__(self):
        return int(self.lengths.shape[0])

    @staticmethod
    def fits(feature_list, device, fraction: float = 0.5) -> bool:
        """True when the packed set takes at most `fraction` of the device's currently free memory."""
        dev = torch.device(device)
        if dev.type != "cuda" or len(feature_list) == 0:
            return False
        _, total = plan_packed_set([int(f.shape[-1]) for f in feature_list], int(feature_list[0].shape[0]))
        free, _total = torch.cuda.mem_get_info(dev)
        return total * 4 <= fraction * free

    def batch(self, idx, spans=None, n_tmask: int = 0):
        """The utterances `idx` (any order, repeats allowed) as (x [b, C, T] float32 device view with rows of T_pad = T rounded up
        to 4 frames, T the longest of them; lengths int32[b] on the host; y float32[b] on the device, or None without labels).
        spans: int32 [b, n, 2] = (start, width) per utterance, its n_tmask time spans first, then its channel spans
        (train_dlqueen.draw_spans), or None.  x is zero behind every utterance and inside the spans.  It lives in ONE buffer owned
        by the set: the next batch overwrites it, ordered on torch's current stream behind whatever read this one there."""
        import ctypes as C
        from . import _lib
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
        b = int(idx.shape[0])
        if b == 0:
            raise ValueError("an empty batch")
        if int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError(f"utterance index outside [0, {len(self)})")
        lengths = np.ascontiguousarray(self.lengths[idx])
        src = np.ascontiguousarray(self.offsets[idx])
        n_sp = 0
        if spans is not None:
            spans = np.ascontiguousarray(spans, dtype=np.int32)
            if spans.ndim != 3 or spans.shape[0] != b or spans.shape[2] != 2 or not 0 <= int(n_tmask) <= spans.shape[1]:
                raise ValueError(f"spans must be int32 [b={b}, n >= n_tmask={n_tmask}, 2], got shape {spans.shape}")
            n_sp = int(spans.shape[1])
        n_t = int(n_tmask) if n_sp else 0
        T = int(lengths.max())
        T_pad = -(-T // 4) * 4
        need = b * self.C * T_pad
        ctx = self.ctx
        with torch.cuda.device(ctx.index):
            if self._x is None or self._x.numel() < need:
                self._x = None
                self._x = torch.empty(need, dtype=torch.float32, device=self.set.device)
            nbytes = int(ctx.lib.dfa_dlq_gather_workspace_bytes(b, n_t, n_sp - n_t))
            if nbytes == 0:
                raise ValueError(f"{n_sp} spans per utterance: the batch gather takes at most 16")
            if self._tab is None or self._tab.numel() < nbytes:
                self._tab = None
                self._tab = torch.empty(nbytes, dtype=torch.uint8, device=self.set.device)
            x = self._x[:need].view(b, self.C, T_pad)
            ctx.use_current_stream()
            code = ctx.lib.dfa_dlq_gather_batch(ctx.handle, _lib.ptr(self.set), self.total_floats, C.c_void_p(src.ctypes.data),
                                                C.c_void_p(lengths.ctypes.data), C.c_void_p(spans.ctypes.data) if n_sp else None,
                                                n_t, n_sp - n_t, b, T, self.C, _lib.ptr(x), self.C * T_pad, T_pad,
                                                _lib.ptr(self._tab), self._tab.numel())
            _lib.check(ctx.handle, code)
            y = None if self.labels is None else self.labels.index_select(0, torch.from_numpy(idx).to(self.set.device))
        return x[:, :, :T], lengths, y


def open_flat(features_path: str, labels_path: str | None, cache_dir: str, rank: int = 0, world: int = 1, tag: str = "set"):
    """(features tensor [N,180,321] zero-copy over a memory-mapped flat file, labels [N] float32 or None, uttids) for the
    data-parallel drivers.  `features_path` is either a flat prefix made by `python -m dfa_amd.ingest` (<prefix>.npy +
    <prefix>.json: nothing is un-pickled by anyone) or the reference's features.pkl: then RANK 0 ALONE converts it once into
    `cache_dir/<tag>_flat.*` (ingest.convert), the other ranks wait at a barrier and map the result -- instead of every rank
    un-pickling, stacking and pinning the whole set."""
    import os
    from . import ingest
    import torch.distributed as dist
    if os.path.exists(features_path + ".npy") and os.path.exists(features_path + ".json"):
        prefix = features_path
    else:
        prefix = os.path.join(cache_dir, f"{tag}_flat")
        if rank == 0:
            os.makedirs(cache_dir, exist_ok=True)
            ingest.convert(features_path, prefix, labels_path, dtype="fp32")
        if world > 1 and dist.is_available() and dist.is_initialized():
            dist.barrier()
    ff = ingest.FlatFeatures(prefix)
    return ff.tensor(), ff.labels, ff.uttids


class RaggedBatcher:
    """Iterate (features, labels, lengths) over a list of per-utterance [F, T_i] tensors of unequal lengths (the layout a
    features.pkl holds), for `model(features, lengths=lengths)`.

    features: [b, T_pad, F] on `device`, the transposed view of a [b, F, T_pad] batch zero-padded to the batch's longest
    utterance (T_pad rounded up so every stored row is a multiple of 16 bytes), staged in pinned memory when `device` is a GPU;
    labels: [b] on `device` or None; lengths: int32 [b] on the CPU.  rank/world shard the utterances contiguously like
    FlatBatcher.  Each utterance's output is independent of its batch companions, so a shard is walked in order of length
    (longest first) to cut padding; `restore` puts per-batch outputs back in input order.

    shuffle_seed (training): every pass over the batcher is a new epoch with its own batches.  The shard is permuted by a
    generator seeded with (shuffle_seed, epoch), cut into buckets of `bucket` utterances (rounded to whole batches; default 16
    batches), each bucket is sorted by length (longest first) and cut into batches -- companions are similar in length, yet
    change from epoch to epoch -- and the batch order is shuffled.  Every utterance appears exactly once per epoch; `batches`
    (and `restore`) describe the latest pass.  shuffle_seed=None: the fixed longest-first order above.
    """

    def __init__(self, features, labels=None, batch_size: int = 32, device="cuda", rank: int = 0, world: int = 1,
                 dtype: torch.dtype | None = None, *, shuffle_seed: int | None = None, bucket: int | None = None):
        n = len(features)
        per = -(-n // world)
        self.lo, self.hi = min(rank * per, n), min((rank + 1) * per, n)
        self.features, self.labels = features, labels
        self.batch_size, self.device, self.dtype = batch_size, torch.device(device), dtype
        F = {int(f.shape[0]) for f in features[self.lo:self.hi]}
        if len(F) > 1:
            raise ValueError(f"ragged utterances must share the feature dimension, got {sorted(F)}")
        lens = np.array([int(f.shape[-1]) for f in features[self.lo:self.hi]], dtype=np.int64)
        self.order = self.lo + np.argsort(-lens, kind="stable")          # longest first, ties in input order
        self.batches = [self.order[i:i + batch_size] for i in range(0, len(self.order), batch_size)]
        self.shuffle_seed, self.epoch = shuffle_seed, 0
        nb = 16 if bucket is None else max(1, -(-int(bucket) // batch_size))       # batches per bucket
        self.bucket = nb * batch_size
        self._lens = lens

    def __len__(self):
        return len(self.batches)

    def _shuffled_batches(self, epoch: int):
        rng = np.random.default_rng([int(self.shuffle_seed), int(epoch)])
        perm = rng.permutation(self.hi - self.lo)
        batches = []
        for b0 in range(0, len(perm), self.bucket):
            part = perm[b0:b0 + self.bucket]
            part = part[np.argsort(-self._lens[part], kind="stable")]
            batches += [self.lo + part[i:i + self.batch_size] for i in range(0, len(part), self.batch_size)]
        return [batches[i] for i in rng.permutation(len(batches))]

    def __iter__(self):
        pin = self.device.type == "cuda"
        if self.shuffle_seed is not None:
            self.batches = self._shuffled_batches(self.epoch)
            self.epoch += 1
        for idx in self.batches:
            utts = [torch.as_tensor(self.features[i]) for i in idx]
            dtype = self.dtype or utts[0].dtype
            lengths = torch.tensor([u.shape[-1] for u in utts], dtype=torch.int32)
            align = max(1, 16 // torch.empty(0, dtype=dtype).element_size())
            t_pad = -(-int(lengths.max()) // align) * align
            host = torch.zeros((len(idx), utts[0].shape[0], t_pad), dtype=dtype, pin_memory=pin)
            for j, u in enumerate(utts):
                host[j, :, :u.shape[-1]] = u
            x = host.to(self.device, non_blocking=True).transpose(1, 2)
            y = None if self.labels is None else torch.as_tensor(np.asarray(self.labels)[idx]).to(self.device)
            yield x, y, lengths

    def restore(self, outputs):
        """Per-batch outputs (first dimension = the batch's utterances, in iteration order) -> one tensor in input order."""
        cat = torch.cat(list(outputs))
        inv = torch.from_numpy(np.argsort(np.concatenate(self.batches) - self.lo, kind="stable")).to(cat.device)
        return cat[inv]


class EvalBatches:
    """One face for both inference sources: a stacked [N, F, T] tensor (FlatBatcher) or a list of per-utterance [F, T_i] tensors
    of unequal lengths (RaggedBatcher).  Iterates (x [b, T, F] on `device`, lengths): lengths is None for a stacked source --
    the model is then called without `lengths=` -- and x its transposed view (the stored batch itself with swap_tf=False);
    `restore` puts per-batch outputs back in input order."""

    def __init__(self, source, batch_size: int, device="cuda", rank: int = 0, world: int = 1, dtype=None, swap_tf: bool = True):
        self.ragged, self.swap_tf = isinstance(source, (list, tuple)), swap_tf
        self.batcher = (RaggedBatcher if self.ragged else FlatBatcher)(source, None, batch_size, device=device, rank=rank,
                                                                      world=world, dtype=dtype)
        self.restore = self.batcher.restore

    def __iter__(self):
        if self.ragged:
            for x, _, lengths in self.batcher:
                yield x, lengths
        else:
            for feats, _ in self.batcher:
                yield (feats.transpose(1, 2) if self.swap_tf else feats), None        # src/predict.py:104-105
