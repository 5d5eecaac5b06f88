"""A graph handle (expann_graph*) driven from NumPy, under the engine: expann_graph_create from the flattened arrays
of a graph_build_helpers.Strided, expann_graph_adopt_build_state with parameters of the caller's choice,
expann_graph_append with levels of the caller's choice, expann_graph_remove, expann_graph_reserve, and the state read
back in the Strided layout.  With it: THE GRAPH REMOVE RULE applied to a Strided (graph_remove_helpers.remove_core on
the `layers` form), and the gather kernel's chunking restated for the preconditions of the tests.

Nothing here needs a device except Handle."""
import ctypes as C

import numpy as np

import graph_remove_helpers as grh
import oracle_ctypes as oc
from graph_build_helpers import Params, Strided, draw_levels

PAD = np.uint64(2 ** 64 - 1)


def make_state(vec, levels, upper_idx, U, L, M, M0, ids0, d0, deg0, idsu, du, degu, max_layer, sv):
    """a Strided over arrays that exist already (row strides = their second dimension)"""
    st = Strided.__new__(Strided)
    st.vec = np.ascontiguousarray(vec, np.float32)
    st.n, st.dim = st.vec.shape
    st.levels = np.ascontiguousarray(levels, np.uint8)
    st.upper_idx = np.ascontiguousarray(upper_idx, np.int32)
    st.M, st.M0, st.U, st.L = M, M0, int(U), int(L)
    st.ids0, st.d0, st.deg0 = ids0, d0, deg0
    st.idsu, st.du, st.degu = idsu, du, degu
    st.stride0, st.strideu = ids0.shape[1], idsu.shape[1]
    st.max_layer, st.sv = int(max_layer), int(sv)
    return st


def _degrees(st, layer):
    """(vertices of level >= layer, their rows in the layer's arrays, min(deg, cap) of each)"""
    if layer == 0:
        return np.arange(st.n), np.arange(st.n), np.minimum(st.deg0[:st.n], st.M0)
    vs = np.flatnonzero(st.levels[:st.n] >= layer)
    rows = (layer - 1) * st.U + st.upper_idx[vs].astype(np.int64)
    return vs, rows, np.minimum(st.degu[rows], st.M)


def flatten(st, n_layers):
    """(layer_offsets uint64 [n_layers][n + 1] into neighbours, neighbours uint32) as expann_graph_create takes them
    and antitopo_index::flatten() makes them: layer-major, a row = its first min(deg, cap) ids in order"""
    off = np.zeros((n_layers, st.n + 1), np.uint64)
    parts, total = [], 0
    for l in range(n_layers):
        vs, rows, deg = _degrees(st, l)
        full = np.zeros(st.n, np.int64)
        full[vs] = deg
        off[l, 0] = total
        off[l, 1:] = total + np.cumsum(full)
        ids = st.ids0 if l == 0 else st.idsu
        parts.append(ids[rows][np.arange(ids.shape[1])[None, :] < deg[:, None]])
        total += int(full.sum())
    nb = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(nb)


def edge_count(st):
    """the sum of min(deg, cap) over every row: what "append_edges" counts"""
    return int(sum(int(_degrees(st, l)[2].sum()) for l in range(st.max_layer)))


def to_layers(st):
    """layers[v][l] = (ids uint64[], lengths float32[]), a row cut at its cap: the form remove_core works on"""
    out = []
    for v in range(st.n):
        per = [(st.ids0[v, :min(int(st.deg0[v]), st.M0)].astype(np.uint64), st.d0[v, :min(int(st.deg0[v]), st.M0)].copy())]
        for l in range(1, int(st.levels[v]) + 1):
            r = st.urow(l, v)
            deg = min(int(st.degu[r]), st.M)
            per.append((st.idsu[r, :deg].astype(np.uint64), st.du[r, :deg].copy()))
        out.append(per)
    return out


def from_layers(vec, layers, M, M0, stride0, strideu, max_layer, sv, new_levels=()):
    """the Strided of a graph in the `layers` form, with empty rows for the vertices to come (their levels:
    new_levels; vec holds their rows too).  upper_idx is the rank among the vertices of level >= 1."""
    levels = np.concatenate([np.array([len(p) - 1 for p in layers], np.uint8), np.asarray(new_levels, np.uint8)])
    st = Strided(vec, levels, M, M0, stride0=stride0, strideu=strideu)
    for v, per in enumerate(layers):
        for l, (ids, d) in enumerate(per):
            if l == 0:
                st.ids0[v, :len(ids)], st.d0[v, :len(ids)], st.deg0[v] = ids, d, len(ids)
            else:
                r = st.urow(l, v)
                st.idsu[r, :len(ids)], st.du[r, :len(ids)], st.degu[r] = ids, d, len(ids)
    st.max_layer, st.sv = int(max_layer), int(sv)
    return st


def extended(st, new_rows, new_levels):
    """the same graph in arrays sized for the rows to come as well: what an append's reference starts from"""
    new_rows = np.ascontiguousarray(new_rows, np.float32)
    return from_layers(np.concatenate([st.vec[:st.n], new_rows]), to_layers(st), st.M, st.M0, st.stride0, st.strideu,
                       st.max_layer, st.sv, new_levels)


def strided_remove(st, ids, keep_cap, p, only=None, select=None):
    """THE GRAPH REMOVE RULE on a Strided: (the Strided it leaves, remove_core's dict).  With only= the rows that were
    not restated are empty in the Strided and None in the dict."""
    gone = np.zeros(st.n, bool)
    gone[np.asarray(ids, np.int64)] = True
    want = grh.remove_core(to_layers(st), st.vec[:st.n], gone, st.M, st.M0, keep_cap, np.float32(p.ortho_factor),
                           np.float32(p.ortho_bias), p.prune_overflow, only=only, select=select)
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.float32))
    layers = [[row if row is not None else empty for row in per] for per in want["layers"]]
    after = from_layers(want["rows"], layers, st.M, st.M0, st.stride0, st.strideu, want["max_layer"], want["starting_vertex"])
    return after, want


def assert_state_is(st, want):
    """a read-back state holds exactly what remove_core returned: levels, upper_idx, top, every id in order and every
    length bit (rows that only= left out are skipped)"""
    assert (st.n, st.max_layer, st.sv) == (want["n"], want["max_layer"], want["starting_vertex"])
    assert np.array_equal(st.vec.view(np.uint32), want["rows"].view(np.uint32))
    levels = np.array([len(p) - 1 for p in want["layers"]])
    assert np.array_equal(st.levels, levels)
    up = levels >= 1
    assert st.U == int(up.sum()) and np.array_equal(st.upper_idx, np.where(up, np.cumsum(up) - 1, -1))
    for v, (got, exp) in enumerate(zip(to_layers(st), want["layers"])):
        for l, ((gi, gd), e) in enumerate(zip(got, exp)):
            if e is None:
                continue
            assert np.array_equal(gi, e[0]), (v, l, gi, e[0])
            assert np.array_equal(gd.view(np.uint32), e[1].view(np.uint32)), (v, l)


def pending_profile(layers, gone):
    """{(vertex, layer): (chunks, distinct candidates, a vertex adopted in two different chunks, pending candidates
    with repeats)} of every touched row, by the gather kernel's chunking (graph_remove_helpers.pending_chunks)"""
    out = {}
    for v in np.flatnonzero(~gone):
        for l, (nb, _) in enumerate(layers[v]):
            nb = nb.astype(np.int64)
            if not gone[nb].any():
                continue
            chunks = grh.pending_chunks(layers, gone, int(v), l)
            sets = [set(c.tolist()) for c in chunks]
            seen, twice = set(), False
            for s in sets:
                twice = twice or bool(seen & s)
                seen |= s
            out[(int(v), l)] = (len(chunks), int((~gone[nb]).sum()) + len(seen), twice, int(sum(len(c) for c in chunks)))
    return out


def batches(levels, n, n_built, max_layer):
    """the batches THE BATCH RULE (max_batch = 0) cuts [n_built, n) into, the top rising as insert_with_level raises it"""
    count, b0 = 0, n_built
    while b0 < n:
        b1 = oc.graph_batch_end(levels, n, b0, max_layer, 0)
        max_layer = max(max_layer, int(np.max(levels[b0:b1])) + 1)
        count, b0 = count + 1, b1
    return count


class Handle:
    """an expann_graph* made from a built Strided.  Keeps the rows on the host (the device state holds none)."""

    def __init__(self, st, M=None, M0=None, ef_construction=None, prune_overflow=0, ortho_factor=0.5, ortho_bias=0.0,
                 adopt=True):
        from expann_amd import _lib
        self._lib = _lib
        self.L = _lib.load()
        self.vec = np.ascontiguousarray(st.vec[:st.n], np.float32)
        self.M, self.M0 = M or st.M, M0 or st.M0
        off, nb = flatten(st, st.max_layer)
        self.h = C.c_void_p()
        rc = self.L.expann_graph_create(st.dim, 0, self.vec.ctypes.data, st.n, st.max_layer, st.sv, off.ctypes.data,
                                        nb.ctypes.data, C.byref(self.h))
        assert rc == 0, (rc, self.L.expann_graph_last_error(None))
        self.max_layer, self.sv = st.max_layer, st.sv
        if adopt:
            rc = self.adopt(st, ef_construction, prune_overflow, ortho_factor, ortho_bias)
            assert rc == 0, (rc, self.error())

    def adopt(self, st, ef_construction, prune_overflow=0, ortho_factor=0.5, ortho_bias=0.0, M=None, M0=None):
        """expann_graph_adopt_build_state with st's arrays: the return code"""
        vp = lambda a: a.ctypes.data
        return self.L.expann_graph_adopt_build_state(
            self.h, M or self.M, M0 or self.M0, ef_construction, prune_overflow, ortho_factor, ortho_bias, vp(st.levels),
            vp(st.upper_idx), vp(st.ids0), vp(st.d0), vp(st.deg0), st.stride0, st.U, st.L, vp(st.idsu), vp(st.du),
            vp(st.degu), st.strideu)

    def error(self):
        return self.L.expann_graph_last_error(self.h)

    def append(self, rows, levels):
        """(return code, rows appended)"""
        rows = np.ascontiguousarray(rows, np.float32)
        levels = np.ascontiguousarray(levels, np.uint8)
        ml, sv, done = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        rc = self.L.expann_graph_append(self.h, rows.ctypes.data, len(rows), levels.ctypes.data, C.byref(ml), C.byref(sv),
                                        C.byref(done))
        if rc == 0:
            self.vec = np.concatenate([self.vec, rows[:done.value]])
            self.max_layer, self.sv = ml.value, sv.value
        return rc, done.value

    def remove(self, ids):
        """(return code, rows removed)"""
        ids = np.ascontiguousarray(ids, np.uint64)
        ml, sv, done = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
        rc = self.L.expann_graph_remove(self.h, ids.ctypes.data, len(ids), C.byref(ml), C.byref(sv), C.byref(done))
        if rc == 0:
            keep = np.ones(len(self.vec), bool)
            keep[ids.astype(np.int64)] = False
            self.vec = np.ascontiguousarray(self.vec[keep])
            self.max_layer, self.sv = ml.value, sv.value
        return rc, done.value

    def reserve(self, n):
        return self.L.expann_graph_reserve(self.h, n)

    def stat(self, name):
        out = C.c_uint64(0)
        assert self.L.expann_graph_get_stat(self.h, name.encode(), C.byref(out)) == 0, name
        return int(out.value)

    def search(self, q, k, ef):
        """(ids uint64 [m][k], distance bits uint32 [m][k], distcomps uint32 [m]) of the plain fp32 walk"""
        q = np.ascontiguousarray(q, np.float32)
        ids = np.empty((len(q), k), np.uint64)
        dists = np.empty((len(q), k), np.float32)
        dc = np.zeros(len(q), np.uint32)
        rc = self.L.expann_graph_search(self.h, q.ctypes.data, len(q), k, ef, 0, ids.ctypes.data, dists.ctypes.data,
                                        dc.ctypes.data)
        assert rc == 0, (rc, self.error())
        return ids, dists.view(np.uint32), dc

    def read_raw(self):
        """((levels, upper_idx, ids0, d0, deg0, idsu, du, degu), U_stride, n_upper_layers, U) as the handle holds them:
        the upper arrays are [n_upper_layers][U_stride] rows, row (l - 1) * U_stride + upper_idx"""
        shape = (C.c_size_t * 6)()
        assert self.L.expann_graph_build_state_shape(self.h, shape) == 0, self.error()
        n, ustride, L, U, s0, su = (int(x) for x in shape)
        assert n == len(self.vec) and L == self.max_layer - 1 and U <= ustride
        levels, upper_idx = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        ids0, d0, deg0 = np.zeros((n, s0), np.uint32), np.zeros((n, s0), np.float32), np.zeros(n, np.uint32)
        rows = max(1, L * ustride)
        idsu, du, degu = np.zeros((rows, su), np.uint32), np.zeros((rows, su), np.float32), np.zeros(rows, np.uint32)
        arrays = (levels, upper_idx, ids0, d0, deg0, idsu, du, degu)
        rc = self.L.expann_graph_read_build_state(self.h, *(a.ctypes.data for a in arrays))
        assert rc == 0, (rc, self.error())
        return arrays, ustride, L, U

    def read(self):
        """the builder's resident state as a Strided: the upper arrays re-strided from [n_upper_layers][U_stride] rows
        to [(l - 1) * U + upper_idx]"""
        (levels, upper_idx, ids0, d0, deg0, idsu, du, degu), ustride, L, U = self.read_raw()
        nu = max(1, L * U)

        def cut(a):
            if L * U == 0:
                return np.zeros((1,) + a.shape[1:], a.dtype)
            return np.ascontiguousarray(a[:L * ustride].reshape((L, ustride) + a.shape[1:])[:, :U].reshape((nu,) + a.shape[1:]))
        return make_state(self.vec, levels, upper_idx, U, L, self.M, self.M0, ids0, d0, deg0, cut(idsu), cut(du), cut(degu),
                          self.max_layer, self.sv)

    def close(self):
        if self.h:
            self.L.expann_graph_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the inputs of tests/test_gpu_graph_handle_mutations.py and tests/test_graph_handle_model.py ----------------------
def gaussian_graph(seed, n, d, M, M0, build, levels=None):
    """(Strided built by the oracle from vertex 0, the RandomState after the rows and levels were drawn)"""
    rng = np.random.RandomState(seed)
    vec = rng.standard_normal((n, d)).astype(np.float32)
    st = Strided(vec, draw_levels(rng, n, M) if levels is None else levels, M, M0)
    st.oracle_build(n, 1, build)
    return st, rng


def random_ids(rng, n, count):
    return np.sort(rng.choice(n, count, replace=False)).astype(np.uint64)


def streamed_case():
    """800 Gaussian rows, d = 64, M = 32, M0 = 64, built with ef 80 and prune_overflow = 64 -- the leniency that lets
    every layer-0 row fill to M0 = 64 ids (with prune_overflow = 0 the Gaussian rows keep 20 of 64, and no sum of
    degrees passes 1024) -- and 320 rows (40 %) to remove.  (state, ids, queries)"""
    st, rng = gaussian_graph(5002, 800, 64, 32, 64, Params(80, prune_overflow=64))
    ids = random_ids(rng, 800, 320)
    return st, ids, rng.standard_normal((32, 64)).astype(np.float32)


def task_chunk_case():
    """38 000 Gaussian rows, d = 48 (the smallest dim the builder's exact tests use), M = 4, M0 = 8, ef 8, a quarter to
    remove.  (state, ids, queries)"""
    st, rng = gaussian_graph(6001, 38000, 48, 4, 8, Params(8))
    ids = random_ids(rng, 38000, 9500)
    return st, ids, rng.standard_normal((32, 48)).astype(np.float32)


def drawn_case(seed=6003, n=600):
    """n Gaussian rows, d = 64, M = 8, M0 = 16, ef 40, drawn levels.  (state, rng, queries)"""
    st, rng = gaussian_graph(seed, n, 64, 8, 16, Params(40))
    return st, rng, rng.standard_normal((32, 64)).astype(np.float32)


def gone_mask(n, ids):
    gone = np.zeros(n, bool)
    gone[np.asarray(ids, np.int64)] = True
    return gone
