"""Host-side mirror (Python) of the reference's engine interface for the brute-force path.

`GpuBruteForceEngine` has the five operations of the reference's CRTP `ann_engine`
(upstream src/ann_engine.h:16-29: name / param_list / store_vector / build / query_k) with
the meaning `brute_force_engine` gives them (src/brute_force_engine.h:9-46), plus the batch
and device-pointer extensions the GPU path needs.  All compute goes through the C ABI
(include/expann_hip.h); this module only moves pointers.  The C++ mirror a maintainer would
drop into the reference tree is include/expann/gpu_brute_force_engine.h.
"""
import ctypes as C

import numpy as np

from . import _lib

_NP_DTYPE = {_lib.DTYPE_F32: np.float32, _lib.DTYPE_U8: np.uint8, _lib.DTYPE_I8: np.int8,
             _lib.DTYPE_I16: np.int16, _lib.DTYPE_F16: np.float16}
_DTYPE = {"f32": _lib.DTYPE_F32, "u8": _lib.DTYPE_U8, "i8": _lib.DTYPE_I8, "i16": _lib.DTYPE_I16,
          "f16": _lib.DTYPE_F16}
# row types whose queries are fp32 at the ABI (the others take queries of the rows' own type)
_F32_QUERIES = (_lib.DTYPE_F32, _lib.DTYPE_U8, _lib.DTYPE_F16)


def pack_row_filter(allow):
    """A boolean array [n] as the little-endian uint32 words of expann_set_row_filter: bit r & 31 of word
    r >> 5 is allow[r]; the bits past n in the last word are zero.  A pure function."""
    allow = np.asarray(allow).astype(bool).reshape(-1)
    by = np.packbits(allow, bitorder="little")
    out = np.zeros((allow.size + 31) // 32 * 4, dtype=np.uint8)
    out[:by.size] = by
    return out.view("<u4").astype(np.uint32)


class GpuBruteForceEngine:
    """Exact k-NN by a full scan on one MI355X (drop-in for brute_force_engine<float>).

    dtype="f16": the rows are kept as IEEE binary16 (numpy casts what is stored, rounding to nearest even),
    half the device memory of "f32"; queries stay float32 and every result is, bit for bit, that of an "f32"
    engine over rows.astype(np.float16).astype(np.float32)."""

    def __init__(self, dim, metric="l2", dtype="f32", device=0):
        self._L = _lib.load()
        self.dim = int(dim)
        self.metric = {"l2": _lib.METRIC_L2, "ip": _lib.METRIC_IP,
                       "l2_i8_refcompat": _lib.METRIC_L2_I8_REFCOMPAT}[metric]
        self.dtype = _DTYPE[dtype]
        self.device = int(device)
        self._metric_name, self._dtype_name = metric, dtype
        h = C.c_void_p()
        rc = self._L.expann_create(self.dim, self.dtype, self.metric, self.device, C.byref(h))
        _lib.check(None, rc)
        self._h = h
        self._built = False

    # ---- the reference interface (src/ann_engine.h:16-29) ---------------------------
    def name(self):
        return "GPU Brute-Force Engine (MI355X)"

    def param_list(self):
        return {"device": str(self.device), "metric": self._metric_name, "dtype": self._dtype_name}

    def store_vector(self, v):
        """src/brute_force_engine.h:20-22: copies one row; ids are insertion order."""
        self.store_many_vectors(np.asarray(v).reshape(1, -1))

    def store_many_vectors(self, rows):
        """Before build(): expann_add.  After build(): expann_append -- the reference's engine has no frozen state
        (store, build, query, store, query), and neither has this one."""
        rows = np.ascontiguousarray(rows, dtype=_NP_DTYPE[self.dtype])
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        call = self._L.expann_append if self._built else self._L.expann_add
        _lib.check(self._h, call(self._h, rows.ctypes.data, rows.shape[0]))

    def build(self):
        """src/brute_force_engine.h:24-26 (asserts a non-empty index): upload to HBM."""
        _lib.check(self._h, self._L.expann_build(self._h))
        self._built = True

    def append(self, rows):
        """expann_append: rows [n, dim] to a built index.  The new rows get the ids size() + i, and every search
        answers as a freshly built index of all the rows does, bit for bit.  A row filter and row groups are
        cleared (they describe the rows they were set for)."""
        rows = np.ascontiguousarray(rows, dtype=_NP_DTYPE[self.dtype])
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        _lib.check(self._h, self._L.expann_append(self._h, rows.ctypes.data, rows.shape[0]))

    def append_device(self, ptr, n, stream=0):
        """expann_append_device: n rows of the index's dtype in device memory, read in the order of `stream` and
        copied; returns when the index holds them."""
        _lib.check(self._h, self._L.expann_append_device(self._h, C.c_void_p(ptr), int(n), C.c_void_p(stream)))

    def reserve(self, n):
        """expann_reserve: room for at least n rows, so that appends up to there do not reallocate the base.
        Before build() the value is remembered for build()."""
        _lib.check(self._h, self._L.expann_reserve(self._h, int(n)))

    def remove(self, ids):
        """expann_remove: the rows whose ids (as a search returns them: row numbers) are given, in any order, a
        repeated id counting once.  The survivors keep their order and move down to fill the gaps -- the row that had
        id i gets i minus the number of removed ids below i; the caller keeps any external id map -- and every search
        then answers as a freshly built index of the survivors does, bit for bit.  size() drops, the capacity stays
        (later appends use the freed room), a row filter and row groups are cleared.  An id >= size() or a removal of
        every row raises and leaves the index as it was.  During the call the rows take twice their device memory.
        Returns the number of rows removed."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        removed = C.c_size_t(0)
        _lib.check(self._h, self._L.expann_remove(self._h, ids.ctypes.data, ids.size, C.byref(removed)))
        return int(removed.value)

    def remove_device(self, ptr, n, stream=0):
        """expann_remove_device: n uint64 ids in device memory, read in the order of `stream`; returns the number of
        rows removed, after the index holds the survivors (the ids may be freed then)."""
        removed = C.c_size_t(0)
        _lib.check(self._h, self._L.expann_remove_device(self._h, C.c_void_p(ptr), int(n), C.c_void_p(stream),
                                                         C.byref(removed)))
        return int(removed.value)

    def compact_row_filter(self):
        """expann_compact_row_filter: removes every row the row filter in force disallows, as remove() of those ids
        does, and clears the filter -- tombstones made permanent.  Raises when no filter is set or when the filter
        allows no row (the filter then stays).  Returns the number of rows removed."""
        removed = C.c_size_t(0)
        _lib.check(self._h, self._L.expann_compact_row_filter(self._h, C.byref(removed)))
        return int(removed.value)

    def query_k(self, v, k):
        """src/brute_force_engine.h:28-46: ids of the min(k, n) nearest rows, ascending."""
        ids, _ = self.query_k_batch(np.asarray(v).reshape(1, -1), k)
        row = ids[0]
        return [int(x) for x in row[row != np.uint64(2 ** 64 - 1)]]

    # ---- extensions ---------------------------------------------------------------
    def query_k_batch(self, queries, k, groups=None):
        """(ids[m,k] uint64, dists[m,k] float32); short rows padded with 2^64-1 / +inf.
        groups: a uint32 array [m] (host) -- query i returns only rows of the group it names
        (expann_search_grouped after set_row_groups; _lib.GROUP_ANY = every row)."""
        qdt = np.float32 if self.dtype in _F32_QUERIES else _NP_DTYPE[self.dtype]
        queries = np.ascontiguousarray(queries, dtype=qdt)
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"queries must be [m, {self.dim}]")
        m = queries.shape[0]
        ids = np.empty((m, k), dtype=np.uint64)
        dists = np.empty((m, k), dtype=np.float32)
        if groups is not None:
            groups = self._query_groups(groups, m)
            _lib.check(self._h, self._L.expann_search_grouped(self._h, queries.ctypes.data, groups.ctypes.data, m, k,
                                                              ids.ctypes.data, dists.ctypes.data))
            return ids, dists
        _lib.check(self._h, self._L.expann_search(self._h, queries.ctypes.data, m, k,
                                                  ids.ctypes.data, dists.ctypes.data))
        return ids, dists

    @staticmethod
    def _query_groups(groups, m):
        groups = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if groups.size != m:
            raise ValueError(f"groups must be [{m}]")
        return groups

    def set_base_device(self, ptr, n, id_offset=0):
        _lib.check(self._h, self._L.expann_set_base_device(self._h, C.c_void_p(ptr), n, id_offset))

    def search_device(self, q_ptr, m, k, ids_ptr, dists_ptr, stream=0, groups=None):
        """expann_search_device; with groups (a HOST uint32 array [m]) expann_search_grouped_device, which
        returns after `stream` has drained."""
        if groups is not None:
            groups = self._query_groups(groups, m)
            _lib.check(self._h, self._L.expann_search_grouped_device(
                self._h, C.c_void_p(q_ptr), groups.ctypes.data, m, k, C.c_void_p(ids_ptr), C.c_void_p(dists_ptr),
                C.c_void_p(stream)))
            return
        _lib.check(self._h, self._L.expann_search_device(
            self._h, C.c_void_p(q_ptr), m, k, C.c_void_p(ids_ptr), C.c_void_p(dists_ptr),
            C.c_void_p(stream)))

    def range_search(self, queries, radius, max_results):
        """expann_range_search: every row with score <= radius (a scalar, or an array [m] of per-query radii; for
        the inner product the score is -dot).  Returns (ids[m, max_results] uint64, dists[m, max_results] float32,
        counts[m] uint32): counts is the exact number of rows in range, the rows are the min(count, max_results)
        nearest ones, ascending by (score, id), padded with 2^64-1 / +inf.  max_results = 0 only counts.  fp32 and
        fp16 rows; no row filter in force."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"queries must be [m, {self.dim}]")
        m, max_results = queries.shape[0], int(max_results)
        radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (m,)))
        ids = np.empty((m, max_results), dtype=np.uint64)
        dists = np.empty((m, max_results), dtype=np.float32)
        counts = np.zeros(m, dtype=np.uint32)
        nul = C.c_void_p(None)
        _lib.check(self._h, self._L.expann_range_search(
            self._h, queries.ctypes.data, radii.ctypes.data, m, max_results,
            ids.ctypes.data if max_results else nul, dists.ctypes.data if max_results else nul,
            counts.ctypes.data))
        return ids, dists, counts

    @staticmethod
    def range_lims(counts, max_results):
        """CSR offsets [m + 1] of the rows range_search returned: the running sum of min(counts, max_results)."""
        kept = np.minimum(np.asarray(counts, dtype=np.int64), int(max_results))
        return np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)

    def range_search_device(self, q_ptr, radii_ptr, m, max_results, ids_ptr, dists_ptr, counts_ptr, stream=0):
        """expann_range_search_device: queries, radii [m] float32 and the outputs are device pointers (ids_ptr /
        dists_ptr may be 0 where the C call allows NULL); returns after `stream` has drained."""
        _lib.check(self._h, self._L.expann_range_search_device(
            self._h, C.c_void_p(q_ptr), C.c_void_p(radii_ptr), m, int(max_results), C.c_void_p(ids_ptr or None),
            C.c_void_p(dists_ptr or None), C.c_void_p(counts_ptr), C.c_void_p(stream)))

    def sync(self):
        """expann_sync: wait for the searches enqueued under set_option("async_search", 1) and
        report on them (raises if one needs the synchronous retry)."""
        _lib.check(self._h, self._L.expann_sync(self._h))

    def score_ids(self, query, ids, cutoff=float("inf")):
        """quantized_scorer::filter_by_score (src/quantizer.h:20-59): (kept_ids, kept_scores)."""
        qdt = np.float32 if self.dtype in _F32_QUERIES else _NP_DTYPE[self.dtype]
        query = np.ascontiguousarray(query, dtype=qdt)
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        kept = np.empty(ids.size, dtype=np.uint64)
        sc = np.empty(ids.size, dtype=np.float32)
        n = C.c_size_t()
        _lib.check(self._h, self._L.expann_score_ids(self._h, query.ctypes.data, ids.ctypes.data,
                                                     ids.size, cutoff, kept.ctypes.data,
                                                     sc.ctypes.data, C.byref(n)))
        return kept[:n.value], sc[:n.value]

    def set_option(self, name, value):
        """expann_set_option (include/expann_hip.h lists the names); among them the select's "rerank_rounds"
        (int8 filter: 2 = two-round exact re-rank, the default; 1 = one round) and "rerank_stats" (1: count the
        re-scored rows for get_stat("rerank_rows"))."""
        _lib.check(self._h, self._L.expann_set_option(self._h, name.encode(), int(value)))

    def set_row_filter(self, allow):
        """expann_set_row_filter: searches return the nearest among the rows where the boolean array
        allow[n] is true (local row numbers, before id_offset), exactly as an index of those rows would;
        None clears the filter (expann_clear_row_filter).  fp32 and fp16 rows only."""
        if allow is None:
            _lib.check(self._h, self._L.expann_clear_row_filter(self._h))
            return
        words = pack_row_filter(allow)
        _lib.check(self._h, self._L.expann_set_row_filter(self._h, words.ctypes.data, words.size))

    def set_row_filter_device(self, ptr, n_words, stream=0):
        """expann_set_row_filter_device: the same from n_words uint32 words in device memory (the layout of
        pack_row_filter), read in the order of `stream`; returns once the allowed rows are counted."""
        _lib.check(self._h, self._L.expann_set_row_filter_device(self._h, C.c_void_p(ptr), int(n_words),
                                                                 C.c_void_p(stream)))

    def set_row_groups(self, groups):
        """expann_set_row_groups: groups[n] (uint32) names the group of every local row; query_k_batch(...,
        groups=) and search_device(..., groups=) then serve each query from the group it names.  A row labelled
        _lib.GROUP_ANY belongs to no group.  None drops the groups (expann_clear_row_groups).  fp32 / fp16 rows."""
        if groups is None:
            _lib.check(self._h, self._L.expann_clear_row_groups(self._h))
            return
        groups = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        _lib.check(self._h, self._L.expann_set_row_groups(self._h, groups.ctypes.data, groups.size))

    def set_row_groups_device(self, ptr, n, stream=0):
        """expann_set_row_groups_device: the same from n uint32 labels in device memory, read in the order of
        `stream`."""
        _lib.check(self._h, self._L.expann_set_row_groups_device(self._h, C.c_void_p(ptr), int(n), C.c_void_p(stream)))

    def get_stat(self, name):
        """expann_get_stat: "redo_queries", "redo_candidates", "redo_overflows", "spec_rank" (speculative thresholds);
        "i8_sample" (1: the last search's sampled pass ran on the int8 matrix cores);
        "rerank_rows" (rows the last search's selects re-scored exactly; counted under the option "rerank_stats");
        "filter_active" (0 / 1) and "filter_rows" (rows the row filter allows; n when none is set);
        "base_bytes" (device bytes of the rows themselves: n * dim * element size);
        "groups_active", "group_count", and of the last grouped search "group_list_queries", "group_filter_queries",
        "group_any_queries", "group_pad_queries", "group_filter_passes";
        of the last range search "range_list_queries", "range_topk_queries", "range_retries";
        "append_calls", "append_rows", "append_extends", "append_rebuilds", "base_capacity_rows", "base_reallocs" and
        "copies_digest" (a digest of the fp16 copy: equal on an appended and on a freshly built index of the same
        rows; 0 without a copy);
        "remove_calls", "remove_rows" (accepted removes and their rows since create), "remove_compacts" (removes that
        carried the fp16 copy over), "remove_rebuilds" (removes that dropped it or forgot an unusable mark)."""
        v = C.c_uint64(0)
        _lib.check(self._h, self._L.expann_get_stat(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def set_profiling(self, enable=True):
        _lib.check(self._h, self._L.expann_set_profiling(self._h, int(bool(enable))))

    def get_profile(self):
        p = _lib.Profile()
        _lib.check(self._h, self._L.expann_get_profile(self._h, C.byref(p)))
        return {f: (getattr(p, f).decode() if f == "scan_kernel" else getattr(p, f))
                for f, _ in _lib.Profile._fields_}

    def size(self):
        return self._L.expann_size(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.expann_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardedBruteForceEngine:
    """Row-sharded exact k-NN over several GPUs behind ONE handle (expann_sharded_*): rows cut into
    contiguous ranges, one RCCL all-gather of the per-shard top-k, merge in the reference's (score, id)
    order -- results bit-identical to GpuBruteForceEngine.  Two forms:
      ShardedBruteForceEngine(dim, devices=[0, 1, ...])                  in-process, host buffers
      ShardedBruteForceEngine(dim, device=d, rank=r, world=G, unique_id=b)   one process per GPU"""

    def __init__(self, dim, metric="l2", dtype="f32", devices=None, device=0, rank=None, world=None,
                 unique_id=None):
        self._L = _lib.load()
        self.dim = int(dim)
        self.metric = {"l2": _lib.METRIC_L2, "ip": _lib.METRIC_IP,
                       "l2_i8_refcompat": _lib.METRIC_L2_I8_REFCOMPAT}[metric]
        self.dtype = _DTYPE[dtype]
        self._dtype_name = dtype
        h = C.c_void_p()
        if rank is None:
            devs = list(devices if devices is not None else [device])
            arr = (C.c_int * len(devs))(*devs)
            rc = self._L.expann_sharded_create(self.dim, self.dtype, self.metric, arr, len(devs), C.byref(h))
            self.devices, self.rank, self.world = devs, None, len(devs)
        else:
            buf = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
            rc = self._L.expann_sharded_create_rank(self.dim, self.dtype, self.metric, int(device), int(rank),
                                                    int(world), buf, C.byref(h))
            self.devices, self.rank, self.world = [int(device)], int(rank), int(world)
        if rc != _lib.OK:
            raise _lib.ExpannError(rc, self._L.expann_sharded_last_error(None).decode())
        self._h = h

    @staticmethod
    def unique_id():
        """128 bytes for the rank form (ncclGetUniqueId); rank 0 makes it, the launcher distributes it."""
        L = _lib.load()
        buf = C.create_string_buffer(128)
        rc = L.expann_sharded_unique_id(buf)
        if rc != _lib.OK:
            raise _lib.ExpannError(rc, L.expann_sharded_last_error(None).decode())
        return buf.raw

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.ExpannError(rc, self._L.expann_sharded_last_error(self._h).decode())

    def name(self):
        return "GPU Brute-Force Engine, row-sharded (MI355X)"

    def param_list(self):
        return {"devices": ",".join(map(str, self.devices)), "shards": str(self.shards()), "dtype": self._dtype_name,
                "exchange": {0: "none", 1: "rccl", 2: "device copies", 3: "caller"}[self.exchange()],
                "exchange_pattern": {0: "none", 1: "all-gather", 2: "all-to-all of query slices"}[self.exchange_pattern()]}

    def store_many_vectors(self, rows):
        rows = np.ascontiguousarray(rows, dtype=_NP_DTYPE[self.dtype])
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        self._check(self._L.expann_sharded_add(self._h, rows.ctypes.data, rows.shape[0]))

    def store_vector(self, v):
        self.store_many_vectors(np.asarray(v).reshape(1, -1))

    def build(self):
        self._check(self._L.expann_sharded_build(self._h))

    def set_shard_device(self, shard, ptr, n, id_offset):
        self._check(self._L.expann_sharded_set_shard_device(self._h, int(shard), C.c_void_p(ptr), n, id_offset))

    def query_k_batch(self, queries, k):
        qdt = np.float32 if self.dtype in _F32_QUERIES else _NP_DTYPE[self.dtype]
        queries = np.ascontiguousarray(queries, dtype=qdt)
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError(f"queries must be [m, {self.dim}]")
        m = queries.shape[0]
        ids = np.empty((m, k), dtype=np.uint64)
        dists = np.empty((m, k), dtype=np.float32)
        self._check(self._L.expann_sharded_search(self._h, queries.ctypes.data, m, k, ids.ctypes.data,
                                                  dists.ctypes.data))
        return ids, dists

    def query_k(self, v, k):
        ids, _ = self.query_k_batch(np.asarray(v).reshape(1, -1), k)
        row = ids[0]
        return [int(x) for x in row[row != np.uint64(2 ** 64 - 1)]]

    def search_device(self, q_ptr, m, k, ids_ptr, dists_ptr, stream=0):
        self._check(self._L.expann_sharded_search_device(self._h, C.c_void_p(q_ptr), m, k, C.c_void_p(ids_ptr),
                                                         C.c_void_p(dists_ptr), C.c_void_p(stream)))

    def search_devices(self, q_ptrs, m, k, ids_ptrs, dists_ptrs):
        """expann_sharded_search_devices (in-process form, everything resident): q_ptrs[r] = the m queries
        on shard r's device; shard r leaves its merged query slice (self.slice(m, r)) at ids_ptrs[r] /
        dists_ptrs[r].  Deferred by default: sync() waits for every device and validates."""
        n = len(q_ptrs)
        arr = lambda ps: (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in ps])
        self._check(self._L.expann_sharded_search_devices(self._h, arr(q_ptrs), m, k, arr(ids_ptrs), arr(dists_ptrs)))

    def slice(self, m, shard):
        """[lo, hi): the queries shard `shard` merges (exchange pattern 2, search_devices)."""
        lo, hi = C.c_size_t(), C.c_size_t()
        self._check(self._L.expann_sharded_slice(self._h, m, int(shard), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def sync(self):
        self._check(self._L.expann_sharded_sync(self._h))

    def exchange_pattern(self):
        """0 none, 1 all-gather of whole chunks, 2 all-to-all of query slices"""
        return self._L.expann_sharded_exchange_pattern(self._h)

    def comm_ranks(self):
        """ranks of the RCCL communicator as ncclCommCount reports them (0: no communicator)"""
        return self._L.expann_sharded_comm_ranks(self._h)

    def last_enqueue_ms(self):
        return self._L.expann_sharded_last_enqueue_ms(self._h)

    def set_alltoallv_fn(self, fn):
        """Rank form: fn(d_send, send_off, send_bytes, d_recv, recv_off, recv_bytes, rank, world, stream)
        -> 0 (lists of `world` ints; entry [rank] is 0 bytes) moves the query slices of exchange pattern 2
        in place of RCCL's send / recv groups (expann_sharded_set_alltoallv_fn); None = RCCL again."""
        if fn is None:
            self._a2afn = _lib.ALLTOALLV_FN(0)
        else:
            def tramp(_ctx, d_send, so, sb, d_recv, ro, rb, rank, world, stream):
                try:
                    return int(fn(d_send or 0, [so[j] for j in range(world)], [sb[j] for j in range(world)],
                                  d_recv or 0, [ro[j] for j in range(world)], [rb[j] for j in range(world)],
                                  rank, world, stream or 0))
                except Exception:  # (an exception cannot cross the C frames above this one)
                    import traceback
                    traceback.print_exc()
                    return 1
            self._a2afn = _lib.ALLTOALLV_FN(tramp)  # (kept alive with the engine)
        self._check(self._L.expann_sharded_set_alltoallv_fn(self._h, self._a2afn, None))

    def set_exchange_fn(self, fn):
        """Rank form: fn(d_send, d_recv, nbytes, rank, world, stream) -> 0 gathers every rank's chunk of
        device memory (expann_sharded_set_exchange_fn) in place of RCCL's all-gather; None = RCCL again."""
        if fn is None:
            self._xfn = _lib.EXCHANGE_FN(0)
        else:
            def tramp(_ctx, d_send, d_recv, nbytes, rank, world, stream):
                try:
                    return int(fn(d_send or 0, d_recv or 0, nbytes, rank, world, stream or 0))
                except Exception:  # (an exception cannot cross the C frames above this one)
                    import traceback
                    traceback.print_exc()
                    return 1
            self._xfn = _lib.EXCHANGE_FN(tramp)  # (kept alive with the engine)
        self._check(self._L.expann_sharded_set_exchange_fn(self._h, self._xfn, None))

    def set_option(self, name, value):
        """expann_set_option (include/expann_hip.h lists the names); among them the select's "rerank_rounds"
        (int8 filter: 2 = two-round exact re-rank, the default; 1 = one round) and "rerank_stats" (1: count the
        re-scored rows for get_stat("rerank_rows"))."""
        self._check(self._L.expann_sharded_set_option(self._h, name.encode(), int(value)))

    def set_profiling(self, enable=True):
        self._check(self._L.expann_sharded_set_profiling(self._h, int(bool(enable))))

    def get_profile(self, shard=0):
        p = _lib.Profile()
        self._check(self._L.expann_sharded_get_profile(self._h, int(shard), C.byref(p)))
        return {f: (getattr(p, f).decode() if f == "scan_kernel" else getattr(p, f))
                for f, _ in _lib.Profile._fields_}

    def size(self):
        return self._L.expann_sharded_size(self._h)

    def shards(self):
        return self._L.expann_sharded_shards(self._h)

    def exchange(self):
        return self._L.expann_sharded_exchange(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.expann_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merge_topk_strided_device(device, in_ids_ptr, in_dists_ptr, ids_stride, dists_stride, n_lists, m,
                              k, out_ids_ptr, out_dists_ptr, stream=0):
    """expann_merge_topk_strided_device: list g at in_ids + g*ids_stride / in_dists + g*dists_stride
    (strides in elements)."""
    L = _lib.load()
    rc = L.expann_merge_topk_strided_device(device, C.c_void_p(in_ids_ptr), C.c_void_p(in_dists_ptr),
                                            ids_stride, dists_stride, n_lists, m, k,
                                            C.c_void_p(out_ids_ptr), C.c_void_p(out_dists_ptr),
                                            C.c_void_p(stream))
    _lib.check(None, rc)


def merge_topk_device(device, in_ids_ptr, in_dists_ptr, n_lists, m, k, out_ids_ptr,
                      out_dists_ptr, stream=0):
    L = _lib.load()
    rc = L.expann_merge_topk_device(device, C.c_void_p(in_ids_ptr), C.c_void_p(in_dists_ptr),
                                    n_lists, m, k, C.c_void_p(out_ids_ptr),
                                    C.c_void_p(out_dists_ptr), C.c_void_p(stream))
    _lib.check(None, rc)
