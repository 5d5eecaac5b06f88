"""Yardstick of the ranged (affine int8) graph walk, composed from the existing oracle:
  * `ranged_convert`: a numpy restatement of the quantiser's convert (tests/test_graph_ranged_abi.py pins it
    against oracle_quantize_ranged_q8 without a GPU);
  * `write_single_layer_index`: an index file in the reference's layout (src/antitopo_engine.h:932-991, the
    layout graph_helpers.read_index_edges documents) whose max_layer is 1, so that the oracle's descent loop
    runs zero times;
  * `ranged_expected`: the oracle's uint8 walk of such a file holding the rows' bytes as floats, asked with
    the queries' bytes as floats -- on bytes the uint8 cast is the identity, so this IS the walk of mode 2 --
    plus the fp32 re-score on the original rows."""
import ctypes as C
import struct

import numpy as np


def oracle_ranged_q8(oracle, rows):
    """(scale_factor float32, offset float32, bytes uint8[n, d]) of oracle_quantize_ranged_q8"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = rows.shape
    out = np.empty((n, d), np.int8)
    scale, offset = C.c_float(), C.c_float()
    oracle.lib().oracle_quantize_ranged_q8(rows.ctypes.data, n, d, out.ctypes.data, C.byref(scale), C.byref(offset))
    return np.float32(scale.value), np.float32(offset.value), out.view(np.uint8)


def ranged_convert(x, scale, offset):
    """fp32 multiply, fp32 add, then floor(float64(r) + 0.5) (= roundf for r > 0), clamped to [0, 127]; 0 for r <= 0"""
    x = np.asarray(x, dtype=np.float32)
    r = (x * np.float32(scale)).astype(np.float32)
    r = (r + np.float32(offset)).astype(np.float32)
    rounded = np.floor(r.astype(np.float64) + 0.5)
    rounded = np.where(r <= 0, 0.0, rounded)
    return np.clip(rounded, 0, 127).astype(np.uint8)


def write_single_layer_index(path, vectors, lists0, starting_vertex, M=16, ef_construction=80):
    """vectors [n][d] fp32 and one bottom-layer list per vertex, max_layer = 1 (edge lengths 0: no reader
    of the query side looks at them)"""
    vectors = np.ascontiguousarray(vectors, dtype=np.float32)
    n, d = vectors.shape
    rec = np.dtype([("d", "<f4"), ("id", "<u8")])
    with open(path, "wb") as f:
        f.write(struct.pack("<QQQQB", starting_vertex, M, 2 * M, 1, 0))
        f.write(struct.pack("<QQffQBBQQ", ef_construction, 1, 0.5, 0.0, 0, 0, 0, 1, n))
        for v in range(n):
            f.write(struct.pack("<Q", d))
            f.write(vectors[v].tobytes())
        f.write(struct.pack("<Q", n))
        for v in range(n):
            e = np.zeros(len(lists0[v]), dtype=rec)
            e["id"] = lists0[v]
            f.write(struct.pack("<QQ", 1, len(e)))
            f.write(e.tobytes())


def build_layer0(lib, rows, tmp_path, M=16, ef_construction=80):
    """serial host build of `rows` through the C ABI at exactly their dim; (starting vertex, layer-0 lists)"""
    from graph_helpers import read_index_edges
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = rows.shape
    h = C.c_void_p()
    assert lib.expann_antitopo_create(d, 0, M, ef_construction, 1, 0, 0, C.byref(h)) == 0
    assert lib.expann_antitopo_store(h, rows.ctypes.data, n) == 0
    path = str(tmp_path / f"built_{n}_{d}.index")
    assert lib.expann_antitopo_save(h, path.encode()) == 0
    lib.expann_antitopo_destroy(h)
    hdr, layers = read_index_edges(path)
    assert hdr["n"] == n
    return hdr["starting_vertex"], [per[0][0] for per in layers]


def graph_create_layer0(lib, rows, lists0, starting_vertex):
    """expann_graph handle over `rows` and the layer-0 lists alone (n_layers = 1)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, d = rows.shape
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists0])
    nb = np.concatenate(lists0).astype(np.uint32)
    h = C.c_void_p()
    rc = lib.expann_graph_create(d, 0, rows.ctypes.data, n, 1, int(starting_vertex), off.ctypes.data, nb.ctypes.data,
                                 C.byref(h))
    assert rc == 0, lib.expann_graph_last_error(None)
    return h


def ranged_expected(oracle, tmp_path, rows, lists0, starting_vertex, q, k, efs):
    """(scale, offset, {ef: (ids, dists, distcomps)}): what mode 2 must return on a one-layer graph"""
    from graph_helpers import read_index_edges
    scale, offset, R = oracle_ranged_q8(oracle, rows)
    path = str(tmp_path / "ranged_bytes.index")
    write_single_layer_index(path, R.astype(np.float32), lists0, starting_vertex)
    hdr, layers = read_index_edges(path)  # the writer against the existing reader
    assert (hdr["max_layer"], hdr["n"], hdr["starting_vertex"]) == (1, len(rows), starting_vertex)
    assert all(len(per) == 1 and np.array_equal(per[0][0], np.asarray(l0, np.uint64))
               for per, l0 in zip(layers, lists0))
    g = oracle.Graph(path)
    assert np.array_equal(g.vectors(), R.astype(np.float32))
    qb = ranged_convert(q, scale, offset).astype(np.float32)
    out = {}
    for ef in efs:
        ids, _, dc = g.query_k(qb, k, ef, True)
        dists = np.full(ids.shape, np.inf, np.float32)
        for i in range(ids.shape[0]):
            for j in range(k):
                if ids[i, j] != np.uint64(2 ** 64 - 1):
                    dists[i, j] = oracle.l2_f32(q[i], rows[int(ids[i, j])])
        out[ef] = (ids, dists, dc)
    return scale, offset, out


def search_mode(lib, h, q, k, ef, mode):
    """(rc, ids, dists, distcomps) of expann_graph_search_mode"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    m = q.shape[0]
    ids = np.zeros((m, k), np.uint64)
    dists = np.zeros((m, k), np.float32)
    dc = np.zeros(m, np.uint32)
    rc = lib.expann_graph_search_mode(h, q.ctypes.data, m, k, ef, mode, ids.ctypes.data, dists.ctypes.data,
                                      dc.ctypes.data)
    return rc, ids, dists, dc
