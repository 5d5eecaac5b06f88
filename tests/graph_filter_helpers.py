"""Yardstick of the graph engine's row filter: a Python restatement of THE FILTER RULE (include/expann_hip.h,
expann_graph_set_row_filter) over an index file in the reference's layout.

  * fp32 distances are oracle.l2_f32's: `dist_f32_matrix` takes them from the oracle's brute force with k = n, which
    scores every (query, row) pair with that very function (tests/test_graph_filter_abi.py compares a sample);
  * byte-mode distances are float32(sum (q8 - r8)^2) over uint8(trunc) bytes in mode 1 and over ranged_convert /
    oracle_ranged_q8 bytes in mode 2 (`dist_bytes_matrix`, exact integers);
  * the two queues are libstdc++'s __push_heap / __adjust_heap restated (`push_heap`, `adjust_heap`, `Heap`): the
    comparators look at the distance only, so the order among equal distances is the heap's
    (tests/test_graph_filter_abi.py replays tests/golden/heap_ref.json through them);
  * `walk` returns ids, distances, distcomps and each query's peak `candidates` size.

Nothing here touches a device, except `graph_from_index`, which uploads an index file for the GPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.uint64(2 ** 64 - 1)


# ---- libstdc++'s heap primitives on parallel lists (d[i], ident[i]) --------------------------------
# less(a, b) on distances only: a max-heap (`nearest`) has less = a < b, a min-heap (`candidates`) less = a > b
def push_heap(d, ident, hole, top, vd, vid, max_heap):
    """std::__push_heap(first, hole, top, value)"""
    while hole > top:
        parent = (hole - 1) // 2
        if not ((d[parent] < vd) if max_heap else (d[parent] > vd)):
            break
        d[hole], ident[hole] = d[parent], ident[parent]
        hole = parent
    d[hole], ident[hole] = vd, vid


def adjust_heap(d, ident, hole, length, vd, vid, max_heap):
    """std::__adjust_heap(first, hole, len, value): the chain of larger children down to a leaf, then __push_heap"""
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if (d[child] < d[child - 1]) if max_heap else (d[child] > d[child - 1]):
            child -= 1
        d[hole], ident[hole] = d[child], ident[child]
        hole = child
    if (length & 1) == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        d[hole], ident[hole] = d[child - 1], ident[child - 1]
        hole = child - 1
    push_heap(d, ident, hole, top, vd, vid, max_heap)


class Heap:
    """std::priority_queue<pair<float, id>> whose comparator looks at .first only"""

    def __init__(self, max_heap, init=()):
        self.max_heap = bool(max_heap)
        self.d = [float(x[0]) for x in init]
        self.id = [int(x[1]) for x in init]
        n = len(self.d)
        if n >= 2:  # std::__make_heap
            for parent in range((n - 2) // 2, -1, -1):
                adjust_heap(self.d, self.id, parent, n, self.d[parent], self.id[parent], self.max_heap)

    def __len__(self):
        return len(self.d)

    def push(self, vd, vid):
        self.d.append(vd)
        self.id.append(vid)
        push_heap(self.d, self.id, len(self.d) - 1, 0, vd, vid, self.max_heap)

    def pop(self):
        n = len(self.d)
        if n > 1:  # std::__pop_heap(first, last - 1, last - 1)
            vd, vid = self.d[n - 1], self.id[n - 1]
            self.d[n - 1], self.id[n - 1] = self.d[0], self.id[0]
            adjust_heap(self.d, self.id, 0, n - 1, vd, vid, self.max_heap)
        self.d.pop()
        self.id.pop()


def heap_trace(max_heap, init, ops):
    """(states, drain) of a queue trace in the format of tests/golden/heap_ref.json"""
    def bits(x):
        return int(np.float32(x).view(np.uint32))
    h = Heap(max_heap, [(float(np.float32(d)), i) for d, i in init])
    state = lambda: (len(h), bits(h.d[0]), h.id[0]) if len(h) else (0, 0, 0)
    states = [state()]
    for kind, d, i in ops:
        if kind == 1:
            h.push(float(np.float32(d)), int(i))
        elif len(h):
            h.pop()
        states.append(state())
    drain = []
    while len(h):
        drain.append((bits(h.d[0]), h.id[0]))
        h.pop()
    return states, drain


# ---- distances ----------------------------------------------------------------------------------
def dist_f32_matrix(oracle, base, q):
    """D[i, v] = oracle.l2_f32(q[i], base[v]) for every pair, through the oracle's brute force with k = n"""
    n = base.shape[0]
    ids, dists = oracle.brute_force(base, q, n, oracle.METRIC_L2_F32, n_threads=4)
    D = np.empty((q.shape[0], n), np.float32)
    np.put_along_axis(D, ids.astype(np.int64), dists, axis=1)
    return D


def dist_bytes_matrix(q8, r8):
    """D[i, v] = float32(sum (q8[i] - r8[v])^2), an exact integer sum"""
    q8, r8 = q8.astype(np.int64), r8.astype(np.int64)
    s = (q8 * q8).sum(1)[:, None] + (r8 * r8).sum(1)[None, :] - 2 * (q8 @ r8.T)
    return s.astype(np.float32)


def bottom_matrix(oracle, base, q, mode, Df):
    """the bottom layer's distances in `mode` (0: Df itself)"""
    if mode == 0:
        return Df
    if mode == 1:  # quantizer_simple<uint8_t>: a plain cast (truncation) of rows and query
        return dist_bytes_matrix(np.trunc(q).astype(np.uint8), np.trunc(base).astype(np.uint8))
    from graph_ranged_helpers import oracle_ranged_q8, ranged_convert
    scale, offset, R = oracle_ranged_q8(oracle, base)
    return dist_bytes_matrix(ranged_convert(q, scale, offset), R)


# ---- the graph ----------------------------------------------------------------------------------
class IndexGraph:
    """adjacency lists per layer of an index file (graph_helpers.read_index_edges), as int64 arrays"""

    def __init__(self, idx):
        from graph_helpers import read_index_edges
        hdr, layers = read_index_edges(idx)
        self.n, self.n_layers, self.sv = hdr["n"], hdr["max_layer"], hdr["starting_vertex"]
        empty = np.zeros(0, np.int64)
        self.adj = [[per[l][0].astype(np.int64) if l < len(per) else empty for per in layers]
                    for l in range(self.n_layers)]

    @classmethod
    def single_layer(cls, lists0, sv):
        g = cls.__new__(cls)
        g.n, g.n_layers, g.sv = len(lists0), 1, int(sv)
        g.adj = [[np.asarray(x).astype(np.int64) for x in lists0]]
        return g


def descent_ends(g, Df):
    """the vertex the greedy descent hands to the bottom layer, per query"""
    return np.array([_descend(g, Df[i])[0] for i in range(Df.shape[0])], np.int64)


def _descend(g, df):
    entry = g.sv
    ep = df[entry]
    dc = 1
    for layer in range(g.n_layers - 1, 0, -1):
        changed = True
        while changed:
            changed = False
            nbs = g.adj[layer][entry]
            dc += len(nbs)
            if len(nbs):
                dn = df[nbs]
                j = int(np.argmin(dn))  # the first occurrence of the minimum: where the first-improvement chain ends
                if dn[j] < ep:
                    ep, entry, changed = dn[j], int(nbs[j]), True
    return entry, dc


def walk_one(g, df, db, allow, k, ef, rescore):
    """THE FILTER RULE for one query.  df[n] / db[n]: its fp32 / bottom-layer distances to every row; allow: bool[n]
    or None (no filter).  (ids list, dists list, distcomps, peak candidates size)"""
    entry, dc = _descend(g, df)
    visited = np.zeros(g.n, bool)
    visited[entry] = True
    cand, near = Heap(False), Heap(True)
    d_entry = float(db[entry])
    dc += 1
    cand.push(d_entry, entry)
    if allow is None or allow[entry]:
        near.push(d_entry, entry)
    peak = 1
    adj0 = g.adj[0]
    while len(cand):
        cd, cur = cand.d[0], cand.id[0]
        if len(near) == ef and cd > near.d[0]:
            break
        cand.pop()
        nbs = adj0[cur]
        fresh = nbs[~visited[nbs]]  # adjacency order
        visited[fresh] = True
        dc += len(fresh)
        dns = db[fresh]
        if len(near) == ef:  # the pre-drop: the top only falls while the queue is full
            keep = dns < near.d[0]
            fresh, dns = fresh[keep], dns[keep]
        ok = np.ones(len(fresh), bool) if allow is None else allow[fresh]
        for nb, dn, a in zip(fresh.tolist(), dns.tolist(), ok.tolist()):
            if len(near) < ef or dn < near.d[0]:
                cand.push(dn, nb)
                if len(cand) > peak:
                    peak = len(cand)
                if a:
                    near.push(dn, nb)
                    if len(near) > ef:
                        near.pop()
    out_d, out_id = [], []
    while len(near):
        out_d.append(near.d[0])
        out_id.append(near.id[0])
        near.pop()
    out_d.reverse()
    out_id.reverse()
    out_d, out_id = out_d[:k], out_id[:k]
    if rescore:
        out_d = [float(df[v]) for v in out_id]
    return out_id, out_d, dc, peak


def walk(g, Df, Db, allow, k, ef, mode):
    """all queries: (ids[m, k] uint64 padded, dists[m, k] float32 padded, distcomps[m] uint64, peak[m] int64)"""
    m = Df.shape[0]
    ids = np.full((m, k), PAD, np.uint64)
    dists = np.full((m, k), np.inf, np.float32)
    dc = np.zeros(m, np.uint64)
    peak = np.zeros(m, np.int64)
    for i in range(m):
        oi, od, dc[i], peak[i] = walk_one(g, Df[i], Db[i], allow, k, ef, mode != 0)
        ids[i, :len(oi)] = oi
        dists[i, :len(od)] = od
    return ids, dists, dc, peak


def reachable_allowed(g, allow, start):
    """allowed vertices that the bottom layer reaches from `start`"""
    seen = np.zeros(g.n, bool)
    seen[start] = True
    stack = [int(start)]
    while stack:
        v = stack.pop()
        for nb in g.adj[0][v].tolist():
            if not seen[nb]:
                seen[nb] = True
                stack.append(nb)
    return int((seen & allow).sum())


# ---- the cases ----------------------------------------------------------------------------------
def sift_like(rng, n, d, frac=False):
    """integer rows in [0, 255] (the uint8 cast is exact on them); frac: queries with fractional parts"""
    x = np.clip(np.round(np.abs(rng.standard_normal((n, d))) * 40.0), 0, 255).astype(np.float32)
    if frac:
        x = np.minimum(255.5, x + rng.uniform(0, 0.99, size=x.shape)).astype(np.float32)
    return x


N_ROWS, M_ALL, M_FILTER, K = 3000, 300, 48, 10
FILTER_NAMES = ("ones", "every_second", "random_10", "block", "no_entry", "last_word_set")


def make_filters(n, ends, sv, seed=7):
    """{name: (allow bool[n], words uint32[] as the caller passes them)}; `ends`: the vertices the descent ends on"""
    from expann_amd import pack_row_filter
    rng = np.random.RandomState(seed)
    f = {}
    f["ones"] = np.ones(n, bool)
    f["every_second"] = np.arange(n) % 2 == 0
    f["random_10"] = rng.rand(n) < 0.10
    blk = np.zeros(n, bool)
    blk[1000:1300] = True
    f["block"] = blk
    ne = np.ones(n, bool)  # `nearest` starts empty: neither the starting vertex nor any end of the descent
    ne[np.asarray(ends, np.int64)] = False
    ne[sv] = False
    f["no_entry"] = ne
    f["last_word_set"] = rng.rand(n) < 0.5
    out = {}
    for name, allow in f.items():
        words = pack_row_filter(allow)
        if name == "last_word_set":  # bits beyond n set in the caller's last word: they must be ignored
            assert n % 32 != 0
            words = words.copy()
            words[-1] = np.uint32(0xFFFFFFFF)
            allow = allow.copy()
            allow[(n // 32) * 32:] = True
        out[name] = (allow, words)
    return out


# ---- an index file without a device ---------------------------------------------------------------
def build_index_cpu(tmp, base, M=16, ef_construction=80, name="cpu"):
    """the serial host builder (include/expann/antitopo_index.h) through tests/native/serial_index_hook.cpp: the index
    file expann_antitopo_store + expann_antitopo_save write, made without a device"""
    so = os.path.join(str(tmp), "serial_index_hook.so")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O3", "-march=x86-64-v3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "native", "serial_index_hook.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.serial_index.restype = C.c_int
    lib.serial_index.argtypes = [C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_char_p]
    base = np.ascontiguousarray(base, dtype=np.float32)
    idx = os.path.join(str(tmp), f"{name}_{base.shape[0]}_{base.shape[1]}.index")
    assert lib.serial_index(base.shape[1], base.ctypes.data, base.shape[0], M, ef_construction, idx.encode()) == 0
    return idx


def graph_from_index(L, idx, vectors):
    """expann_graph handle over an index file: every layer's lists as CSR, layer l at row l of the offsets"""
    from graph_helpers import read_index_edges
    hdr, layers = read_index_edges(idx)
    n, n_layers = hdr["n"], hdr["max_layer"]
    off = np.zeros((n_layers, n + 1), np.uint64)
    nbs, base = [], 0
    for layer in range(n_layers):
        deg = np.array([len(per[layer][0]) if layer < len(per) else 0 for per in layers], np.uint64)
        off[layer, 0] = base
        off[layer, 1:] = base + np.cumsum(deg)
        nbs += [per[layer][0] for per in layers if layer < len(per)]
        base += int(deg.sum())
    nb = np.concatenate(nbs).astype(np.uint32)
    vectors = np.ascontiguousarray(vectors, dtype=np.float32)
    h = C.c_void_p()
    rc = L.expann_graph_create(vectors.shape[1], 0, vectors.ctypes.data, n, n_layers, hdr["starting_vertex"],
                               off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    return h
