"""THE GRAPH REMOVE RULE (include/expann_hip.h) restated in NumPy, independent of the C++: an index file in the
reference's layout, the ids to remove -> the adjacency with lengths, max_layer and starting_vertex the rule leaves.

float32 arithmetic throughout.  Pair distances are the oracle's l2_f32 (the reference's 16-lane FMA order), the
ortho term is two rounded operations, prune_edges picks the first of equal scores in (length, id) order."""
import ctypes as C
import struct

import numpy as np

import oracle_ctypes as oc
from graph_helpers import read_index_edges

F32_MAX = np.float32(3.402823466e+38)


def read_index_rows(path):
    """(rows float32 [n][d], ortho_factor, ortho_bias) of an index file"""
    raw = open(path, "rb").read()
    pos = 32
    has_ef = raw[pos]
    pos += 1 + (8 if has_ef else 0)
    pos += 16
    factor, bias = struct.unpack_from("<ff", raw, pos)
    pos += 8 + 8 + 2 + 8
    n, = struct.unpack_from("<Q", raw, pos)
    pos += 8
    d, = struct.unpack_from("<Q", raw, pos)
    rec = np.frombuffer(raw, dtype=np.dtype([("len", "<u8"), ("v", "<f4", (d,))]), count=n, offset=pos)
    assert (rec["len"] == d).all()
    return np.ascontiguousarray(rec["v"]), np.float32(factor), np.float32(bias)


class _Dist:
    """oracle_l2_f32 between rows of one array, by row number"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.base = self.rows.ctypes.data
        self.step = self.rows.strides[0]
        self.d = self.rows.shape[1]
        self.fn = oc.lib().oracle_l2_f32
        self.memo = {}

    def __call__(self, a, b):
        key = (a, b) if a < b else (b, a)
        r = self.memo.get(key)
        if r is None:
            r = np.float32(self.fn(C.c_void_p(self.base + key[0] * self.step), C.c_void_p(self.base + key[1] * self.step), self.d))
            self.memo[key] = r
        return r


def prune_edges(cand, limit, dist, factor, bias, prune_overflow):
    """prune_edges(l, v, lazy=false) over `cand` = [(length float32, id)] sorted by (length, id)"""
    alive = [[d, i, d, prune_overflow + 1] for d, i in cand]   # basic, id, score so far, leniency
    ret = []
    while len(ret) < limit and alive:
        best = 0
        for j in range(1, len(alive)):
            if alive[j][2] < alive[best][2]:
                best = j
        if alive[best][2] == F32_MAX:
            break
        basic_b, id_b, _, _ = alive.pop(best)
        ret.append((basic_b, id_b))
        if len(ret) == limit:
            break
        for c in alive:
            if c[2] == F32_MAX:
                continue
            co = dist(id_b, c[1])
            if co < c[0]:
                term = np.float32(factor * np.float32(c[0] - co))
                c[2] = np.float32(c[2] + np.float32(term + bias))
                c[3] -= 1
                if c[3] == 0:
                    c[2] = F32_MAX
    return ret


def apply_remove(index_path, ids):
    """dict(layers=[v][l] -> (ids uint64[], lengths float32[]) under the new ids, max_layer, starting_vertex, n,
    touched, truncated, empty_rows (touched rows that ended empty), rows)"""
    hdr, layers = read_index_edges(index_path)
    rows, factor, bias = read_index_rows(index_path)
    n = hdr["n"]
    gone = np.zeros(n, bool)
    gone[np.asarray(ids, np.uint64).astype(np.int64)] = True
    assert not gone.all()
    keep_cap = max(hdr["ef_construction"], hdr["M0"])
    dist = _Dist(rows)
    new_id = np.cumsum(~gone) - 1
    out, touched, truncated, empty = [], 0, 0, 0
    for v in range(n):
        if gone[v]:
            continue
        per = []
        for l, (nb, ln) in enumerate(layers[v]):
            nb = nb.astype(np.int64)
            lost = gone[nb]
            if not lost.any():
                per.append((new_id[nb].astype(np.uint64), ln.copy()))
                continue
            touched += 1
            cand = {int(i): np.float32(d) for i, d in zip(nb[~lost], ln[~lost])}
            for r in nb[lost]:
                for c in layers[r][l][0].astype(np.int64):
                    c = int(c)
                    if gone[c] or c == v or c in cand:
                        continue
                    cand[c] = dist(v, c)
            lst = sorted((d, i) for i, d in cand.items())
            if len(lst) > keep_cap:
                truncated += 1
                lst = lst[:keep_cap]
            kept = prune_edges(lst, hdr["M0"] if l == 0 else hdr["M"], dist, factor, bias, hdr["prune_overflow"])
            empty += not kept
            per.append((np.array([new_id[i] for _, i in kept], np.uint64), np.array([d for d, _ in kept], np.float32)))
        out.append(per)
    levels = np.array([len(p) for p in out])
    top = int(levels.max())
    return dict(layers=out, max_layer=top, starting_vertex=int(np.nonzero(levels == top)[0][0]), n=len(out),
                touched=touched, truncated=truncated, empty_rows=empty, rows=rows[~gone])


def assert_file_is(path, want):
    """the index file at `path` holds exactly what apply_remove returned: header, rows, every edge and length bit"""
    hdr, layers = read_index_edges(path)
    rows, _, _ = read_index_rows(path)
    assert (hdr["n"], hdr["max_layer"], hdr["starting_vertex"]) == (want["n"], want["max_layer"], want["starting_vertex"])
    assert np.array_equal(rows.view(np.uint32), want["rows"].view(np.uint32))
    assert len(layers) == want["n"]
    for v, (got, exp) in enumerate(zip(layers, want["layers"])):
        assert len(got) == len(exp), (v, len(got), len(exp))
        for l, ((gi, gd), (ei, ed)) in enumerate(zip(got, exp)):
            assert np.array_equal(gi, ei), (v, l, gi, ei)
            assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), (v, l)
