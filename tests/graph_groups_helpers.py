"""Yardstick of the graph engine's row groups (THE GROUP RULE, include/expann_hip.h): per query, either
graph_filter_helpers.walk_one with allow = (labels == the query's group) -- None for EXPANN_GROUP_ANY --, the
restatement tests/test_graph_filter_abi.py pins to the oracle and to libstdc++'s heaps; or, for a query the rule
sends to the scan, the min(k, s) smallest (Df[i, v], v) over the group's rows with distcomps s; or padding.  The
serve decision (group_serve, csrc/graph_search.hpp) is restated in `serve`.

Nothing here touches a device, except `graph_f16_from_index`."""
import ctypes as C

import numpy as np

import graph_filter_helpers as H

ANY = 0xFFFFFFFF
TOP = 0xFFFFFFFE  # the largest legal key
ABSENT = 12345    # a group no row carries
QUERY_CYCLE = (5, 2, 1, TOP, 3, 9, ANY, ABSENT)
FLAT_AUTO, FLAT_MAX_KEYS = 128000, 1024
N_ROWS, M, K, EFS = H.N_ROWS, H.M_FILTER, H.K, (10, 40)
WALK, SCAN, PAD = "walk", "scan", "pad"


def make_labels(n=N_ROWS, seed=11):
    """rows 1000..1299 -> TOP (a block); 7 random rows -> 3 (fewer than k); 1 row -> 9; 40 rows -> 0xFFFFFFFF (no
    group); of the rest: even rows -> 5, about 10 % of the odd rows -> 1, the other odd rows -> 2"""
    rng = np.random.RandomState(seed)
    idx = np.arange(n)
    lab = np.where(idx % 2 == 0, 5, np.where(rng.rand(n) < 0.10, 1, 2)).astype(np.uint32)
    lab[1000:1300] = TOP
    outside = np.concatenate([idx[:1000], idx[1300:]])
    pick = rng.choice(outside, 7 + 1 + 40, replace=False)
    lab[pick[:7]] = 3
    lab[pick[7]] = 9
    lab[pick[8:]] = ANY
    return lab


def other_labels(n=N_ROWS):
    """a second labelling with the same keys on other rows: thirds of the rows"""
    return (np.arange(n) * 3 // n).astype(np.uint32) * 2 + 1  # 1, 3, 5


def query_groups(m=M):
    return np.array([QUERY_CYCLE[i % len(QUERY_CYCLE)] for i in range(m)], np.uint32)


def group_size(labels, qg):
    return 0 if qg == ANY else int((labels == np.uint32(qg)).sum())


def serve(s, k, flat_rows):
    """how a query whose group has s rows is served at "filter_flat_rows" = flat_rows (0 = auto)"""
    F = FLAT_AUTO if flat_rows == 0 else flat_rows
    if s == 0:
        return PAD
    if s <= F and min(k, s) <= FLAT_MAX_KEYS:
        return SCAN
    return WALK


def classify(labels, qgroups, k, flat_rows):
    """per query: WALK / SCAN / PAD (an ANY query walks)"""
    return [WALK if int(qg) == ANY else serve(group_size(labels, int(qg)), k, flat_rows) for qg in qgroups]


def check_classes(labels, qgroups, ends):
    """the class sizes the tests rely on; ends: the vertex each query's descent ends on"""
    size = {int(x): group_size(labels, int(x)) for x in set(QUERY_CYCLE) - {ANY}}
    assert size[TOP] == 300 and 100 <= size[1] < 400, size       # scanned at 400, walked at 1
    assert size[5] > 1000 and size[2] > 1000, size               # walked at 400
    assert size[3] == 7 and size[9] == 1 and size[ABSENT] == 0, size
    assert int((labels == np.uint32(ANY)).sum()) == 40
    assert sorted(set(labels.tolist())) == [1, 2, 3, 5, 9, TOP, ANY]
    outside = [i for i, qg in enumerate(qgroups) if int(qg) != ANY and size[int(qg)] and labels[ends[i]] != qg]
    assert outside, "no query's descent ends outside its group"
    return size


def scan_one(df, labels, qg, k):
    """(ids, dists, distcomps) of the exact scan of group qg for one query: the min(k, s) smallest (distance, id)"""
    rows = np.flatnonzero(labels == np.uint32(qg))
    order = np.lexsort((rows, df[rows]))[:min(k, rows.size)]  # distances are >= 0 and finite: their order is their bits'
    return rows[order].tolist(), df[rows[order]].tolist(), int(rows.size)


class Restatement:
    """expected answers of grouped searches over one graph; walks are computed once per (query, group, mode, ef)"""

    def __init__(self, g, Df, Db_of_mode):
        self.g, self.Df, self.Db_of_mode, self._walks = g, Df, Db_of_mode, {}

    def _walk(self, i, qg, labels_key, labels, mode, ef, k):
        key = (i, qg, labels_key, mode, ef, k)
        if key not in self._walks:
            allow = None if qg == ANY else labels == np.uint32(qg)
            self._walks[key] = H.walk_one(self.g, self.Df[i], self.Db_of_mode(mode)[i], allow, k, ef, mode != 0)
        return self._walks[key]

    def expected(self, labels, qgroups, k, ef, mode, flat_rows, labels_key="main"):
        """(ids[m, k] uint64 padded, dists[m, k] float32 padded, distcomps[m] uint64, classes, peak candidates of
        the walked queries)"""
        m = len(qgroups)
        ids = np.full((m, k), H.PAD, np.uint64)
        dists = np.full((m, k), np.inf, np.float32)
        dc = np.zeros(m, np.uint64)
        peaks = {}
        classes = classify(labels, qgroups, k, flat_rows)
        for i, (qg, cl) in enumerate(zip(qgroups.tolist(), classes)):
            if cl == PAD:
                continue
            if cl == SCAN:
                oi, od, dc[i] = scan_one(self.Df[i], labels, qg, k)
            else:
                oi, od, dc[i], peaks[i] = self._walk(i, qg, labels_key, labels, mode, ef, k)
            ids[i, :len(oi)] = oi
            dists[i, :len(od)] = od
        return ids, dists, dc, classes, peaks


def graph_f16_from_index(L, idx, vectors):
    """expann_graph_create_f16 handle over an index file; the rows must be exact in binary16"""
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
    halves = np.ascontiguousarray(vectors, dtype=np.float16)
    assert np.array_equal(halves.astype(np.float32), vectors)
    h = C.c_void_p()
    rc = L.expann_graph_create_f16(vectors.shape[1], 0, halves.ctypes.data, n, n_layers, hdr["starting_vertex"],
                                   off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    return h
