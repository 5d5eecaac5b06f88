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


def dist_block(rows, a, b):
    """D[i][j] = the oracle's l2_f32(rows[a[i]], rows[b[j]]): one oracle call for the whole block"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    D = np.empty((len(a), len(b)), np.float32)
    if len(a) and len(b):
        ids, dists = oc.brute_force(rows[b], rows[a], len(b))
        np.put_along_axis(D, ids.astype(np.int64), dists, axis=1)
    return D


def prune_list(d, ids, limit, rows, factor, bias, prune_overflow):
    """prune_edges over the candidates (d[i], ids[i]) sorted by (length, id), the pair distances from one oracle call
    and the scores as float32 arrays: [(length, id)] as prune_edges returns it"""
    if len(ids) == 0:
        return []
    lazy = len(ids) > 2 * limit   # (a long list: only the rows of the picks are ever read)
    D = None if lazy else dist_block(rows, ids, ids)
    d = np.asarray(d, np.float32)
    score = d.copy()
    left = np.full(len(ids), prune_overflow + 1)
    gone = np.zeros(len(ids), bool)
    factor, bias = np.float32(factor), np.float32(bias)
    ret = []
    while len(ret) < limit:
        best = int(np.argmin(np.where(gone, np.inf, score)))   # (the first of equal scores)
        if gone[best] or score[best] == F32_MAX:
            break
        gone[best] = True
        ret.append((d[best], int(ids[best])))
        if len(ret) == limit:
            break
        co = dist_block(rows, ids[best:best + 1], ids)[0] if lazy else D[best]
        hit = ~gone & (score != F32_MAX) & (co < d)
        term = (factor * (d[hit] - co[hit]).astype(np.float32)).astype(np.float32)
        score[hit] = (score[hit] + (term + bias).astype(np.float32)).astype(np.float32)
        left[hit] -= 1
        score[hit & (left == 0)] = F32_MAX
    return ret


def pending_chunks(layers, gone, v, l):
    """the adopted candidates of the touched row (v, l) in the chunks the gather kernel takes them in: the removed
    neighbours in row order, a new chunk when the degrees of a chunk's rows would sum past 1024.  A list of id arrays,
    repeats kept; a candidate is a surviving neighbour of a removed neighbour that is neither v nor an own entry."""
    nb = layers[v][l][0].astype(np.int64)
    own = set(nb[~gone[nb]].tolist())
    chunks, cur, bound = [], [], 0
    for r in nb[gone[nb]]:
        ids_r = layers[r][l][0].astype(np.int64)
        if bound + len(ids_r) > 1024:
            chunks.append(cur)
            cur, bound = [], 0
        bound += len(ids_r)
        cur.extend(c for c in ids_r[~gone[ids_r]].tolist() if c != v and c not in own)
    chunks.append(cur)
    return [np.asarray(c, np.int64) for c in chunks]


def remove_core(layers, rows, gone, M, M0, keep_cap, factor, bias, prune_overflow, only=None, select=None):
    """THE GRAPH REMOVE RULE on arrays: layers[v][l] = (ids, lengths float32) of the graph before, rows float32 [n][d],
    gone bool [n].  only: the touched (old vertex, layer) rows to restate -- the others come back as None, and are
    still counted.  select(own, chunks, cap) -> ([(length, id)], truncated) replaces the rule's choice of candidates
    (own = [(length, id)], chunks = [[(length, id)]] with repeats): the wrong variants of tests/test_graph_handle_model.py.
    Returns apply_remove's dict."""
    n = len(layers)
    assert not gone.all()
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
            chunks = pending_chunks(layers, gone, v, l)
            adopted = np.unique(np.concatenate(chunks))
            if only is not None and (v, l) not in only:
                truncated += int(lost.size - lost.sum()) + len(adopted) > keep_cap
                per.append(None)
                continue
            d_ad = dist_block(rows, [v], adopted)[0]
            if select is None:
                ids = np.concatenate([nb[~lost], adopted])
                d = np.concatenate([ln[~lost], d_ad])
                order = np.lexsort((ids, d))
                cut = len(order) > keep_cap
                ids, d = ids[order[:keep_cap]], d[order[:keep_cap]]
            else:
                length = dict(zip(adopted.tolist(), d_ad))
                lst, cut = select(list(zip(ln[~lost], nb[~lost].tolist())), [[(length[c], c) for c in ch.tolist()] for ch in chunks],
                                  keep_cap)
                d, ids = np.array([x for x, _ in lst], np.float32), np.array([i for _, i in lst], np.int64)
            truncated += bool(cut)
            kept = prune_list(d, ids, M0 if l == 0 else M, rows, factor, bias, prune_overflow)
            empty += not kept
            per.append((np.array([new_id[i] for _, i in kept], np.uint64), np.array([x for x, _ in kept], np.float32)))
        out.append(per)
    levels = np.array([len(p) for p in out])
    top = int(levels.max())
    return dict(layers=out, max_layer=top, starting_vertex=int(np.nonzero(levels == top)[0][0]), n=len(out),
                touched=touched, truncated=truncated, empty_rows=empty, rows=rows[~gone])


def apply_remove(index_path, ids):
    """dict(layers=[v][l] -> (ids uint64[], lengths float32[]) under the new ids, max_layer, starting_vertex, n,
    touched, truncated, empty_rows (touched rows that ended empty), rows)"""
    hdr, layers = read_index_edges(index_path)
    rows, factor, bias = read_index_rows(index_path)
    gone = np.zeros(hdr["n"], bool)
    gone[np.asarray(ids, np.uint64).astype(np.int64)] = True
    return remove_core(layers, rows, gone, hdr["M"], hdr["M0"], max(hdr["ef_construction"], hdr["M0"]), factor, bias,
                       hdr["prune_overflow"])


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
