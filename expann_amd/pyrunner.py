"""Python module surface of the reference (upstream src/pyrunner.cpp:41-91) over the C ABI:
`AntitopoEngine(M, ef_construction, ortho_count, prune_overflow, use_compression)` with
store_vector / store_many_vectors(array2d, take_norms) / build / query_k / query_k_numpy /
set_ef_search / name / param_list, plus `query_many` (batched) and index save/load.

The reference compiles one module per dimension (expann_py_64/128/256/832/960,
CMakeLists.txt:102-153) and zero-pads every row to that DIM (src/pyrunner.cpp:20-27); here the
dimension is a constructor argument (default: from the first rows -- up to 960 the smallest dim
with a compiled graph kernel that holds them, from 961 to 4096 the next multiple of 64, so that
every compression mode works) and rows are zero-padded the same way.  Wider rows raise ValueError.  take_norms = L2-normalise each row before
storing (angular data = normalise + L2, src/pyrunner.cpp:78-79); the normalisation itself is
Eigen's in the reference (summation order unpinned) and numpy float32 here.

`use_compression` also takes "ranged" (and `set_compression("none" | "cast" | "ranged")` switches a live
engine): the bottom layer walks an int8 copy of the rows made by one global affine quantiser (the
reference's quantizer_ranged_q8, src/quantizer.h:152-238, which it never runs), so rows that are not
integers in [0, 255] -- Gaussian, embeddings, take_norms=True -- get a compressed walk too.  True / False
keep the reference's meaning (the uint8 cast / fp32).

`rows="f16"` keeps the rows as IEEE binary16 on the device (expann_antitopo_set_rows_f16): every stored float is
rounded to the nearest-even binary16 as it comes in, the builders and the index file see the rounded values, and the
walk gathers half the bytes.  Rows with a NaN or a value beyond binary16's range are refused.
"""
import ctypes as C

import numpy as np

from . import _lib

_SUPPORTED_DIMS = (64, 128, 256, 512, 768, 832, 960)  # dims with compiled graph kernels
_MAX_DIM = 4096  # the graph path's limit (run-time-dim kernels above 960)
_COMPRESSION_MODES = {"none": _lib.GRAPH_FP32, "cast": _lib.GRAPH_U8_CAST, "ranged": _lib.GRAPH_RANGED_Q8}


def _compression_mode(value):
    """expann_graph_compression of a use_compression / set_compression argument"""
    if isinstance(value, str):
        if value not in _COMPRESSION_MODES:
            raise ValueError(f"compression must be one of {sorted(_COMPRESSION_MODES)}, not {value!r}")
        return _COMPRESSION_MODES[value]
    return _lib.GRAPH_U8_CAST if value else _lib.GRAPH_FP32


class AntitopoEngine:
    def __init__(self, M, ef_construction, ortho_count, prune_overflow, use_compression, dim=None,
                 device=0, rows="f32"):
        if rows not in ("f32", "f16"):
            raise ValueError(f'rows must be "f32" or "f16", not {rows!r}')
        self._rows_f16 = rows == "f16"
        self._mode = _compression_mode(use_compression)
        if self._mode == _lib.GRAPH_RANGED_Q8 and dim is not None and int(dim) % 64 != 0:
            raise ValueError(f"the ranged walk needs a dimension that is a multiple of 64, not {dim}")
        self._L = _lib.load()
        # (the handle is created with the reference's flag: "ranged" is a run-time mode set on top of it)
        self._args = (int(M), int(ef_construction), int(ortho_count), int(prune_overflow),
                      self._mode == _lib.GRAPH_U8_CAST)
        self.device = int(device)
        self.dim = None
        self._h = None
        if dim is not None:
            self._open(int(dim))

    def _open(self, dim):
        if dim > _MAX_DIM:
            raise ValueError(f"dimension {dim} exceeds the graph engine's limit of {_MAX_DIM}")
        padded = next((d for d in _SUPPORTED_DIMS if d >= dim), None)
        if padded is None:
            padded = (dim + 63) // 64 * 64
        h = C.c_void_p()
        M, efc, oc, po, uc = self._args
        rc = self._L.expann_antitopo_create(padded, self.device, M, efc, oc, po, int(uc), C.byref(h))
        if rc != _lib.OK:
            raise _lib.ExpannError(rc, self._L.expann_antitopo_last_error(None).decode())
        self._h, self.dim = h, padded
        if self._rows_f16:
            self._check(self._L.expann_antitopo_set_rows_f16(h, 1))
        if self._mode != int(uc):
            self._check(self._L.expann_antitopo_set_compression(h, self._mode))

    def _check(self, rc):
        if rc != _lib.OK:
            raise _lib.ExpannError(rc, self._L.expann_antitopo_last_error(self._h).decode())

    def _pad(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2:
            raise RuntimeError("Input should be a 2D NumPy array")  # src/pyrunner.cpp:64-66
        if self._h is None:
            self._open(a.shape[1])
        if a.shape[1] > self.dim:
            raise ValueError("row longer than the engine dimension")
        if a.shape[1] < self.dim:  # convert_raw_to_eigen_padded, src/pyrunner.cpp:20-27
            p = np.zeros((a.shape[0], self.dim), dtype=np.float32)
            p[:, :a.shape[1]] = a
            a = p
        return a

    # ---- the reference's methods ------------------------------------------------------
    def name(self):
        return "GPU Anti-Topo Engine+ (MI355X)"

    def param_list(self):
        M, efc, oc, po, uc = self._args
        pl = {"M": str(M), "M0": str(2 * M), "ef_construction": str(efc), "ortho_count": str(oc),
              "prune_overflow": str(po), "use_compression": str(int(self._mode != _lib.GRAPH_FP32)),
              "num_distcomps": str(self._L.expann_antitopo_num_distcomps(self._h) if self._h else 0)}
        if self._mode == _lib.GRAPH_RANGED_Q8:
            pl["compression_mode"] = "ranged"
        if self._rows_f16:
            pl["rows"] = "f16"
        return pl

    def store_vector(self, v):
        self.store_many_vectors(np.asarray(v, dtype=np.float32).reshape(1, -1), False)

    def store_many_vectors(self, array2d, take_norms):
        a = self._pad(array2d)
        if take_norms:
            a = a / np.sqrt(np.einsum("ij,ij->i", a, a, dtype=np.float32))[:, None]
            a = np.ascontiguousarray(a, dtype=np.float32)
        self._check(self._L.expann_antitopo_store(self._h, a.ctypes.data, a.shape[0]))

    def store_many_vectors_batched(self, array2d, take_norms=False, n_serial=2048):
        """store_many_vectors through the batched GPU builder (csrc/graph_build.hpp): the first
        n_serial rows of an empty engine are inserted serially, the rest in batches on the GPU."""
        a = self._pad(array2d)
        if take_norms:
            a = a / np.sqrt(np.einsum("ij,ij->i", a, a, dtype=np.float32))[:, None]
            a = np.ascontiguousarray(a, dtype=np.float32)
        self._check(self._L.expann_antitopo_store_batched(self._h, a.ctypes.data, a.shape[0], int(n_serial)))

    def build(self):
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_INVALID_ARG, "build() on an empty index")
        self._check(self._L.expann_antitopo_build(self._h))

    def query_k(self, v, k):
        ids, _ = self.query_many(np.asarray(v, dtype=np.float32).reshape(1, -1), k)
        row = ids[0]
        return [int(x) for x in row[row != np.uint64(2 ** 64 - 1)]]

    def query_k_numpy(self, array1d, k):
        return self.query_k(array1d, k)

    def set_ef_search(self, ef_search):
        self._check(self._L.expann_antitopo_set_ef_search(self._h, int(ef_search)))

    # ---- extensions ------------------------------------------------------------------
    def set_compression(self, mode):
        """Bottom-layer scoring of the queries from now on: "none" (fp32), "cast" (the reference's uint8
        cast) or "ranged" (the affine int8 quantiser).  The index and its file do not change."""
        if not isinstance(mode, str):
            raise ValueError('compression must be "none", "cast" or "ranged"')
        m = _compression_mode(mode)
        if self._h is not None:
            self._check(self._L.expann_antitopo_set_compression(self._h, m))
        self._mode = m

    def query_many(self, queries, k, groups=None):
        """groups: None, or one uint32 per query -- the row group it may return (set_row_groups; _lib.GROUP_ANY:
        every row)"""
        if groups is not None and self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "query_many(groups=) before build()")
        q = self._pad(queries)
        ids = np.empty((q.shape[0], k), dtype=np.uint64)
        dists = np.empty((q.shape[0], k), dtype=np.float32)
        if groups is None:
            self._check(self._L.expann_antitopo_query(self._h, q.ctypes.data, q.shape[0], k,
                                                      ids.ctypes.data, dists.ctypes.data))
            return ids, dists
        qg = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        if qg.size != q.shape[0]:
            raise ValueError("groups must hold one uint32 per query")
        self._check(self._L.expann_antitopo_query_grouped(self._h, q.ctypes.data, qg.ctypes.data, q.shape[0], k,
                                                          ids.ctypes.data, dists.ctypes.data))
        return ids, dists

    def query_many_device(self, q_ptr, m, k, ids_ptr, dists_ptr, stream=0, groups_ptr=0):
        """query_many on device buffers, enqueued on `stream` (a hipStream_t as an integer; 0 = the engine's own)
        without waiting for it: q_ptr -> m rows of float32 that ALREADY have the engine's padded `dim` (there is no
        padding on this path), ids_ptr -> uint64 [m][k], dists_ptr -> float32 [m][k], raw device addresses (a torch
        tensor's data_ptr()).  The same sticky ef_search and compression mode as query_many.  The results are valid
        after sync(); searches of one engine overlap only in stream order.  groups_ptr != 0 -> m uint32 in device
        memory: the row group each query may return (set_row_groups)."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "query_many_device() before build()")
        if groups_ptr:
            self._check(self._L.expann_antitopo_query_grouped_device(self._h, C.c_void_p(q_ptr), C.c_void_p(groups_ptr),
                                                                     int(m), int(k), C.c_void_p(ids_ptr),
                                                                     C.c_void_p(dists_ptr), C.c_void_p(stream or None)))
            return
        self._check(self._L.expann_antitopo_query_device(self._h, C.c_void_p(q_ptr), int(m), int(k),
                                                         C.c_void_p(ids_ptr), C.c_void_p(dists_ptr),
                                                         C.c_void_p(stream or None)))

    def range_search(self, queries, radius, max_results):
        """expann_antitopo_range_query: per query the rows within `radius` (squared L2; a scalar, or an array [m] of
        per-query radii) that the walk scored -- THE RANGE WALK RULE, include/expann_hip.h.  Returns
        (ids[m, max_results] uint64, dists[m, max_results] float32, counts[m] uint32): the rows are the
        min(in range and kept, max_results) nearest ones the walk kept, ascending, padded with 2^64-1 / +inf; counts
        is the number of in-range rows the walk scored -- never more than the true number, and more than max_results
        when a row was truncated.  Approximate, as the walk is: every returned row is truly in range, not every
        in-range row is found.  max_results = 0 only counts.  The sticky ef_search of query_many; fp32 bottom layer
        whatever the compression mode; no row filter in force."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "range_search() before build()")
        q = self._pad(queries)
        m, max_results = q.shape[0], int(max_results)
        radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32), (m,)))
        ids = np.empty((m, max_results), dtype=np.uint64)
        dists = np.empty((m, max_results), dtype=np.float32)
        counts = np.zeros(m, dtype=np.uint32)
        nul = C.c_void_p(None)
        self._check(self._L.expann_antitopo_range_query(
            self._h, q.ctypes.data, radii.ctypes.data, m, max_results, ids.ctypes.data if max_results else nul,
            dists.ctypes.data if max_results else nul, counts.ctypes.data))
        return ids, dists, counts

    def range_search_device(self, q_ptr, radii_ptr, m, max_results, ids_ptr, dists_ptr, counts_ptr, stream=0):
        """range_search on device buffers, enqueued on `stream` (a hipStream_t as an integer; 0 = the engine's own)
        without waiting: q_ptr -> m rows of float32 of the engine's padded `dim`, radii_ptr -> float32 [m], ids_ptr ->
        uint64 [m][max_results], dists_ptr -> float32 [m][max_results] (0 where the C call allows NULL), counts_ptr ->
        uint32 [m].  The results are valid after sync()."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "range_search_device() before build()")
        self._check(self._L.expann_antitopo_range_query_device(
            self._h, C.c_void_p(q_ptr), C.c_void_p(radii_ptr), int(m), int(max_results), C.c_void_p(ids_ptr or None),
            C.c_void_p(dists_ptr or None), C.c_void_p(counts_ptr), C.c_void_p(stream or None)))

    def set_row_filter(self, allow):
        """expann_antitopo_set_row_filter: queries from now on return only rows where the boolean (or 0 / 1 uint8)
        array allow[size()] is true; None clears the filter.  Dense filters are walked under the filter rule of
        include/expann_hip.h, sparse ones are answered by an exact scan of the allowed rows.  A run-time property:
        store*, build() and load_index() clear it, and it is not saved with the index."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "set_row_filter() before build()")
        if allow is None:
            self._check(self._L.expann_antitopo_set_row_filter(self._h, None, 0))
            return
        from .engine import pack_row_filter
        words = pack_row_filter(allow)
        self._check(self._L.expann_antitopo_set_row_filter(self._h, words.ctypes.data, words.size))

    def set_row_filter_device(self, ptr, n_words, stream=0):
        """The same from n_words uint32 words in device memory (the layout of pack_row_filter), read in the order of
        `stream` (a hipStream_t as an integer; 0 = the engine's own); returns once the allowed rows are counted."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "set_row_filter_device() before build()")
        self._check(self._L.expann_antitopo_set_row_filter_device(self._h, C.c_void_p(ptr), int(n_words),
                                                                  C.c_void_p(stream or None)))

    def set_row_groups(self, groups):
        """expann_antitopo_set_row_groups: groups[size()] uint32, the group of every row (THE GROUP RULE,
        include/expann_hip.h); None clears them.  query_many(..., groups=) then lets every query name the group it
        may return; queries without groups= ignore the labels.  A run-time property: store*, build() and
        load_index() clear it, and it is not saved with the index."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "set_row_groups() before build()")
        if groups is None:
            self._check(self._L.expann_antitopo_set_row_groups(self._h, None, 0))
            return
        g = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        self._check(self._L.expann_antitopo_set_row_groups(self._h, g.ctypes.data, g.size))

    def set_row_groups_device(self, ptr, n, stream=0):
        """The same from n uint32 labels in device memory, read in the order of `stream` (a hipStream_t as an
        integer; 0 = the engine's own)."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "set_row_groups_device() before build()")
        self._check(self._L.expann_antitopo_set_row_groups_device(self._h, C.c_void_p(ptr), int(n),
                                                                  C.c_void_p(stream or None)))

    def sync(self):
        """Wait for the stream of the last query_many_device and check every such search since the last sync()
        (raises ExpannError with ERR_OVERFLOW when a walk overflowed its queue even in the redo launch)."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "sync() before build()")
        self._check(self._L.expann_antitopo_sync(self._h))

    def append(self, rows):
        """expann_antitopo_append: `rows` (2-D, padded like stored rows) join the BUILT graph with the ids size() ..
        size() + len(rows) - 1 -- THE GRAPH APPEND RULE, include/expann_hip.h: the engine is then what
        store_many_vectors_batched(rows) followed by build() would have made of it, without the graph going to the
        device again (fp32 rows, ortho_count 1, at least 2048 rows; other engines take exactly that route).  A row
        filter and row groups are cleared.  Returns the number of rows appended; raises ExpannError with
        ERR_OVERFLOW -- its `appended` attribute says how many rows are in -- when a construction search overflowed."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "append() before build()")
        a = self._pad(rows)
        done = C.c_size_t(0)
        rc = self._L.expann_antitopo_append(self._h, a.ctypes.data, a.shape[0], C.byref(done))
        if rc != _lib.OK:
            err = _lib.ExpannError(rc, self._L.expann_antitopo_last_error(self._h).decode())
            err.appended = int(done.value)
            raise err
        return int(done.value)

    def reserve(self, n):
        """expann_antitopo_reserve: room on the device for n rows in all, so that appends up to there reallocate
        nothing ("capacity_rows"); below the current capacity it does nothing."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "reserve() before build()")
        self._check(self._L.expann_antitopo_reserve(self._h, int(n)))

    def remove(self, ids):
        """expann_antitopo_remove: the rows `ids` (any order, repeats allowed) leave the BUILT graph -- THE GRAPH REMOVE
        RULE, include/expann_hip.h: survivors keep their order (id i becomes i minus the removed ids below i), every
        row that lost a neighbour adopts the surviving neighbours of the neighbours it lost and is pruned again by the
        builder's rule, on the device (fp32 rows, ortho_count 1, at least 2048 rows; other engines take the host's
        statement of the same rule and a re-upload).  size() drops, the capacity stays, a row filter and row groups
        are cleared.  An id >= size() or a removal of every row raises and leaves the engine as it was.  Returns the
        number of rows removed."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "remove() before build()")
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        done = C.c_size_t(0)
        self._check(self._L.expann_antitopo_remove(self._h, a.ctypes.data, a.shape[0], C.byref(done)))
        return int(done.value)

    def compact_row_filter(self):
        """expann_antitopo_compact_row_filter: remove() of the rows the bitmap filter in force disallows -- tombstones
        made permanent.  No filter in force, or one that allows no row, raises; a filter that allows every row removes
        nothing and is cleared.  Returns the number of rows removed."""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "compact_row_filter() before build()")
        done = C.c_size_t(0)
        self._check(self._L.expann_antitopo_compact_row_filter(self._h, C.byref(done)))
        return int(done.value)

    def stat(self, name):
        """expann_antitopo_get_stat: a counter of the engine's graph handle by its expann_graph_get_stat name
        ("append_device", "capacity_rows", "filter_active", ...)"""
        if self._h is None:
            raise _lib.ExpannError(_lib.ERR_NOT_BUILT, "stat() before build()")
        out = C.c_uint64(0)
        self._check(self._L.expann_antitopo_get_stat(self._h, name.encode(), C.byref(out)))
        return int(out.value)

    def save_index(self, path):
        self._check(self._L.expann_antitopo_save(self._h, str(path).encode()))

    def load_index(self, path):
        self._check(self._L.expann_antitopo_load(self._h, str(path).encode()))

    def size(self):
        return self._L.expann_antitopo_size(self._h) if self._h else 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.expann_antitopo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
