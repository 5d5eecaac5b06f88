"""The batched graph builder (expann_graph_build_batched) against the oracle's CPU restatement
(oracle_graph_build_batched): the strided adjacency arrays both work on, the two calls, and the exact
comparison of their results.

What is compared follows from the builder's contract.  Within one batch everything is determined except the
order in which reverse edges are appended to a row: new rows and re-pruned rows are compared in order, every
other row as its old prefix in order plus the appended (id, distance bits) pairs as a sorted list.  No
tolerances anywhere."""
import ctypes as C
import copy

import numpy as np

import oracle_ctypes as oc


def draw_levels(rng, n, M):
    """the reference's level formula (src/antitopo_engine.h:323) over numpy's uniform draws in (0, 1]"""
    u = 1.0 - rng.random_sample(n)
    return np.floor(-np.log(u) / np.log(float(M))).astype(np.uint8)


def sift_like(rng, n, d):
    return np.clip(np.round(np.abs(rng.standard_normal((n, d))) * 40.0), 0, 255).astype(np.float32)


class Params:
    def __init__(self, ef, prune_overflow=0, ortho_factor=0.5, ortho_bias=0.0):
        self.ef, self.prune_overflow, self.ortho_factor, self.ortho_bias = ef, prune_overflow, ortho_factor, ortho_bias


class Strided:
    """vectors, levels and the adjacency arrays of the C ABI, sized for all n rows; vertex 0 built"""

    def __init__(self, vec, levels, M, M0, slack=64, stride0=None, strideu=None):
        self.vec = np.ascontiguousarray(vec, np.float32)
        self.n, self.dim = self.vec.shape
        self.levels = np.ascontiguousarray(levels, np.uint8)
        self.M, self.M0 = M, M0
        self.stride0 = stride0 or M0 + slack
        self.strideu = strideu or M + slack
        up = self.levels >= 1
        self.upper_idx = np.where(up, np.cumsum(up) - 1, -1).astype(np.int32)
        self.U = int(up.sum())
        self.L = int(self.levels.max())
        self.ids0 = np.zeros((self.n, self.stride0), np.uint32)
        self.d0 = np.zeros((self.n, self.stride0), np.float32)
        self.deg0 = np.zeros(self.n, np.uint32)
        nu = max(1, self.U * self.L)
        self.idsu = np.zeros((nu, self.strideu), np.uint32)
        self.du = np.zeros((nu, self.strideu), np.float32)
        self.degu = np.zeros(nu, np.uint32)
        self.max_layer = int(self.levels[0]) + 1
        self.sv = 0

    def copy(self):
        c = copy.copy(self)   # (vec, levels, upper_idx are never written: shared)
        for a in ("ids0", "d0", "deg0", "idsu", "du", "degu"):
            setattr(c, a, getattr(self, a).copy())
        return c

    def urow(self, layer, v):
        return (layer - 1) * self.U + int(self.upper_idx[v])

    def groups(self):
        """(name, ids, distance bits, deg, stride, cap) of layer 0 and of the upper layers"""
        nu = self.U * self.L
        return [("layer0", self.ids0, self.d0.view(np.uint32), self.deg0, self.stride0, self.M0),
                ("upper", self.idsu[:nu], self.du.view(np.uint32)[:nu], self.degu[:nu], self.strideu, self.M)]

    def oracle_build(self, n, n_built, p, max_batch=0):
        r = oc.graph_build_batched(self.vec, n, self.levels, n_built, self.max_layer, self.sv, self.M, self.M0,
                                   p.ef, p.prune_overflow, p.ortho_factor, p.ortho_bias, max_batch, self.ids0,
                                   self.d0, self.deg0, self.upper_idx, self.U, self.L, self.idsu, self.du, self.degu)
        self.max_layer, self.sv = r["max_layer"], r["starting_vertex"]
        return r

    def gpu_build(self, n, n_built, p, max_batch=0):
        from expann_amd import _lib
        L = _lib.load()
        vp, sz = C.c_void_p, C.c_size_t
        ml, sv = C.c_uint32(self.max_layer), C.c_uint32(self.sv)
        stats = np.full(4, 2 ** 64 - 1, np.uint64)
        L.expann_graph_build_batched.restype = C.c_int
        rc = L.expann_graph_build_batched(
            C.c_int(self.dim), C.c_int(0), vp(self.vec.ctypes.data), sz(n), vp(self.levels.ctypes.data), sz(n_built),
            C.byref(ml), C.byref(sv), sz(self.M), sz(self.M0), sz(p.ef), sz(p.prune_overflow),
            C.c_float(p.ortho_factor), C.c_float(p.ortho_bias), sz(max_batch), vp(self.ids0.ctypes.data),
            vp(self.d0.ctypes.data), vp(self.deg0.ctypes.data), sz(self.stride0), vp(self.upper_idx.ctypes.data),
            sz(self.U), sz(self.L), vp(self.idsu.ctypes.data), vp(self.du.ctypes.data), vp(self.degu.ctypes.data),
            sz(self.strideu), vp(stats.ctypes.data))
        assert rc == 0, (rc, L.expann_graph_last_error(None))
        self.max_layer, self.sv = ml.value, sv.value
        return dict(max_layer=ml.value, starting_vertex=sv.value, stats=stats)


def seed_graph(vec, levels, M, M0, n_built, p, **strides):
    """the oracle's own build of the first n_built rows, from vertex 0 alone"""
    st = Strided(vec, levels, M, M0, **strides)
    if n_built > 1:
        st.oracle_build(n_built, 1, p)
    return st


def _pairs(ids, dbits, lo, hi):
    return sorted(zip(ids[lo:hi].tolist(), dbits[lo:hi].tolist()))


def _appended(bef, orc, b0, b1):
    """{group name: {row: [(new vertex, distance bits)]}}: the reverse edges of the batch, from the oracle's new rows"""
    out = {"layer0": {}, "upper": {}}
    for v in range(b0, b1):
        for layer in range(min(int(bef.levels[v]), bef.max_layer - 1) + 1):
            if layer == 0:
                name, row, ids, d = "layer0", v, orc.ids0, orc.d0.view(np.uint32)
                deg = int(orc.deg0[v])
            else:
                name, row, ids, d = "upper", bef.urow(layer, v), orc.idsu, orc.du.view(np.uint32)
                deg = int(orc.degu[row])
            for i in range(deg):
                nb = int(ids[row, i])
                nrow = nb if layer == 0 else bef.urow(layer, nb)
                out[name].setdefault(nrow, []).append((v, int(d[row, i])))
    return out


def compare_batch(bef, gpu, orc, rg, ro, b0, b1, overflow=False):
    """one batch [b0, b1): `bef` the arrays both calls started from, `gpu` / `orc` what they left, rg / ro
    what they returned.  overflow: rows that could not take all their reverse edges are held to the
    invariants only (which edges were dropped depends on the order of the atomics).  Returns the number of
    rows the oracle re-pruned and the number that overflowed."""
    assert (rg["max_layer"], rg["starting_vertex"]) == (ro["max_layer"], ro["starting_vertex"]), (b0, b1)
    assert [int(x) for x in rg["stats"]] == [int(x) for x in ro["stats"]], (b0, b1, rg["stats"], ro["stats"])
    assert int(ro["stats"][0]) == 1
    app = _appended(bef, orc, b0, b1)
    n_over = 0
    for gb, gg, go, ordered in zip(bef.groups(), gpu.groups(), orc.groups(), (ro["ordered0"], ro["orderedu"])):
        name, ids_b, d_b, deg_b, stride, cap = gb
        _, ids_g, d_g, deg_g, _, _ = gg
        _, ids_o, d_o, deg_o, _, _ = go
        nrows = len(ordered)
        ids_b, d_b, deg_b = ids_b[:nrows], d_b[:nrows], deg_b[:nrows]
        ids_g, d_g, deg_g = ids_g[:nrows], d_g[:nrows], deg_g[:nrows]
        ids_o, d_o, deg_o = ids_o[:nrows], d_o[:nrows], deg_o[:nrows]
        over = np.zeros(nrows, bool)
        for row, lst in app[name].items():
            over[row] = int(deg_b[row]) + len(lst) > stride
        if not overflow:
            assert not over.any(), "a row ran out of slack: give the case more"
        n_over += int(over.sum())
        assert np.array_equal(deg_g[~over], deg_o[~over]), (name, b0, np.nonzero((deg_g != deg_o) & ~over)[0][:8])
        live = np.arange(stride)[None, :] < np.minimum(deg_o, stride)[:, None]
        exact = (ordered.astype(bool) | (deg_o == deg_b)) & ~over
        bad = (((ids_g != ids_o) | (d_g != d_o)) & live).any(axis=1) & exact
        assert not bad.any(), (name, b0, b1, "rows differ in order", np.nonzero(bad)[0][:8])
        for row in np.nonzero(~exact & ~over)[0]:   # appended to, not pruned: old prefix + a set
            lo, hi = int(deg_b[row]), int(deg_o[row])
            assert np.array_equal(ids_g[row, :lo], ids_b[row, :lo]) and np.array_equal(d_g[row, :lo], d_b[row, :lo]), (name, row)
            assert _pairs(ids_g[row], d_g[row], lo, hi) == _pairs(ids_o[row], d_o[row], lo, hi) == sorted(app[name][row]), (name, row)
        for row in np.nonzero(over)[0]:
            deg = int(deg_g[row])
            assert deg <= cap, (name, row, deg)
            allowed = dict(_pairs(ids_b[row], d_b[row], 0, min(int(deg_b[row]), stride)))
            allowed.update(dict(app[name][row]))
            got = _pairs(ids_g[row], d_g[row], 0, deg)
            assert len({i for i, _ in got}) == deg, (name, row, "duplicate ids")
            assert all(i in allowed and allowed[i] == d for i, d in got), (name, row)
    return int(ro["stats"][2]), n_over


def drive_batches(st, n, n_built, p, max_batch=0, overflow=False, on_batch=None):
    """the build from n_built to n, one batch per call on both sides, from the oracle's arrays each time.
    Returns (batches, rows re-pruned, rows that overflowed)."""
    b0, batches, repruned, n_over = n_built, 0, 0, 0
    while b0 < n:
        b1 = oc.graph_batch_end(st.levels, n, b0, st.max_layer, max_batch)
        gpu, orc = st.copy(), st.copy()
        rg = gpu.gpu_build(b1, b0, p, max_batch)
        ro = orc.oracle_build(b1, b0, p, max_batch)
        a, b = compare_batch(st, gpu, orc, rg, ro, b0, b1, overflow)
        if on_batch:
            on_batch(st, orc, ro, b0, b1)
        repruned += a
        n_over += b
        batches += 1
        st, b0 = orc, b1
    return st, batches, repruned, n_over


def compare_run(gpu, orc, rg, ro, stat_ids=(0, 2)):
    """a whole multi-batch call: rows whose last change was a prune in order, the others as sets"""
    assert (rg["max_layer"], rg["starting_vertex"]) == (ro["max_layer"], ro["starting_vertex"])
    for i in stat_ids:
        assert int(rg["stats"][i]) == int(ro["stats"][i]), (i, rg["stats"], ro["stats"])
    for gg, go, ordered in zip(gpu.groups(), orc.groups(), (ro["ordered0"], ro["orderedu"])):
        name, ids_g, d_g, deg_g, stride, _ = gg
        _, ids_o, d_o, deg_o, _, _ = go
        nrows = len(ordered)
        assert np.array_equal(deg_g[:nrows], deg_o[:nrows]), name
        for row in range(nrows):
            deg = int(deg_o[row])
            a = list(zip(ids_g[row, :deg].tolist(), d_g[row, :deg].tolist()))
            b = list(zip(ids_o[row, :deg].tolist(), d_o[row, :deg].tolist()))
            if not ordered[row]:
                a, b = sorted(a), sorted(b)
            assert a == b, (name, row)


def restride(st, stride0=None, strideu=None):
    """the same graph in arrays of other row strides"""
    out = copy.copy(st)
    out.stride0, out.strideu = stride0 or st.stride0, strideu or st.strideu
    for ids, d, s_old, s_new in (("ids0", "d0", st.stride0, out.stride0), ("idsu", "du", st.strideu, out.strideu)):
        w = min(s_old, s_new)
        for name in (ids, d):
            a = getattr(st, name)
            b = np.zeros((a.shape[0], s_new), a.dtype)
            b[:, :w] = a[:, :w]
            setattr(out, name, b)
    out.deg0, out.degu = st.deg0.copy(), st.degu.copy()
    assert out.deg0.max() <= out.stride0 and out.degu.max() <= out.strideu
    return out


def contraction_case(d, which):
    """Four rows on an integer lattice on which prune_edges' answer hangs on how ortho_factor * (basic - co) +
    ortho_bias is rounded.  The new vertex 3 sits at the origin; vertex 0 (distance 3) is kept first; vertex 1
    (distance 6, 1 away from vertex 0) then scores 6 + (factor * 5 + bias), vertex 2 (distance 15, no closer
    kept edge) scores 15.  With each operation rounded -- the rule -- case 0 is an exact tie (the first of
    equals, vertex 1, goes next) and case 1 gives 15.000001 (vertex 2 goes next); one fused multiply-add gives
    the other answer in both.  prune_overflow = 1 keeps vertex 1 alive after its one closer edge.
    Returns (vec, Params, the row of vertex 3 under the rule)."""
    vec = np.zeros((4, d), np.float32)
    vec[0, :3] = (1, 1, 1)
    vec[1, :3] = (2, 1, 1)
    vec[2, :4] = (-1, -1, -2, 3)
    factor, bias, row = [(1.7, float.fromhex("0x1.00000cp-1"), [0, 1, 2]),
                         (1.3, float.fromhex("0x1.400006p+1"), [0, 2, 1])][which]
    return vec, Params(8, 1, factor, bias), row
