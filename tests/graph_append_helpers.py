"""Helpers of tests/test_gpu_graph_append.py: a reader of the reference's index file (the layout of
antitopo_index.h::write_index) and the comparison THE GRAPH APPEND RULE is stated in -- size, max_layer,
starting_vertex and every (vertex, layer) row as a sorted list of (distance bits, id), no tolerances."""
import struct

import numpy as np

EDGE = np.dtype([("d", "<u4"), ("id", "<u8")])  # 12 bytes, packed: the distance's bits, the neighbour


def read_index(path):
    raw = open(path, "rb").read()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, raw, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]
    sv, M, M0, _efm = take("QQQQ")
    if take("B"):
        take("Q")
    _efc, _oc, _of, _ob, _po, _uc, _ul, max_layer = take("QQffQBBQ")
    n = take("Q")
    dim = struct.unpack_from("<Q", raw, pos)[0] if n else 0
    rec = np.dtype([("len", "<u8"), ("row", "<f4", (dim,))])
    vec = np.frombuffer(raw, rec, n, pos)
    assert (vec["len"] == dim).all()
    pos += n * rec.itemsize
    assert take("Q") == n
    rows, levels = {}, np.zeros(n, np.int64)
    for v in range(n):
        nl = take("Q")
        levels[v] = nl - 1
        for layer in range(nl):
            ne = take("Q")
            e = np.frombuffer(raw, EDGE, ne, pos)
            pos += ne * EDGE.itemsize
            rows[(v, layer)] = np.sort(e, order=("d", "id")).tobytes()
    assert pos == len(raw)
    return dict(size=n, dim=dim, M=M, M0=M0, max_layer=max_layer, starting_vertex=sv, rows=rows, levels=levels,
                vectors=vec["row"], edges=sum(len(r) for r in rows.values()) // EDGE.itemsize)


def assert_same_index(path_a, path_b):
    """the fields THE GRAPH APPEND RULE names, and the rows' vectors"""
    a, b = read_index(path_a), read_index(path_b)
    for key in ("size", "max_layer", "starting_vertex"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert np.array_equal(a["vectors"].view(np.uint32), b["vectors"].view(np.uint32))
    assert a["rows"].keys() == b["rows"].keys()
    diff = [k for k in a["rows"] if a["rows"][k] != b["rows"][k]]
    assert not diff, f"{len(diff)} (vertex, layer) rows differ, the first: {sorted(diff)[:5]}"
    return a
