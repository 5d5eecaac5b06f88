"""Graph path at run-time dims (any multiple of 16 up to 4096; the uint8 walk at multiples of 64): the
D = 0 instances of graph_search_kernel, build_search_kernel and build_prune_kernel against the oracle's
restatement of the reference -- walk parity (ids, distance bits, distance-evaluation counts), the batched
builder's invariants, the Python surface, and 64-bit row offsets past 2^32 elements."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "expann_amd", "host", "expann_graph_tool")


def _tool(*args):
    if not os.path.exists(TOOL):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(TOOL)])
    out = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    return [json.loads(x) for x in out.stdout.strip().splitlines()]


def _modes(d):
    return (0, 1) if d % 64 == 0 else (0,)


def _read_results(rf, d, m, k, efs):
    """{(comp, ef): (ids, dists, distcomps)} of an expann_graph_tool results file"""
    raw = open(rf, "rb").read()
    pos, out = 0, {}
    for comp in _modes(d):
        for ef in efs:
            ids = np.frombuffer(raw, np.uint64, m * k, pos).reshape(m, k); pos += m * k * 8
            dists = np.frombuffer(raw, np.float32, m * k, pos).reshape(m, k); pos += m * k * 4
            dc = np.frombuffer(raw, np.uint32, m, pos); pos += m * 4
            out[(comp, ef)] = (ids, dists, dc)
    assert pos == len(raw)
    return out


def _sift_like(rng, n, d, frac=False):
    x = np.clip(np.round(np.abs(rng.standard_normal((n, d))) * 40.0), 0, 255).astype(np.float32)
    if frac:  # fractional parts: the uint8 path truncates the query
        x = np.minimum(255.5, x + rng.uniform(0, 0.99, size=x.shape)).astype(np.float32)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", [(16, 1500), (48, 1500), (96, 1500), (192, 1500), (384, 1500), (1024, 1500),
                                 (1536, 1500), (2048, 1000), (4096, 600)])
def test_gpu_walk_at_run_time_dims_matches_oracle(tmp_path, oracle, d, n):
    """serial host build, SIFT-like rows; fp32 walk at every dim, uint8 walk at the multiples of 64"""
    idx, qf, rf = tmp_path / "g.index", tmp_path / "g.queries", tmp_path / "g.results"
    m, k, efs = 64, 10, [10, 25, 60]
    lines = _tool("--n", n, "--m", m, "--d", d, "--k", k, "--M", 16, "--ef_construction", 80, "--data", "sift",
                  "--index", idx, "--queries", qf, "--results", rf, "--ef", ",".join(map(str, efs)))
    assert sum(1 for x in lines if x["phase"] == "query") == len(_modes(d)) * len(efs)
    g = oracle.Graph(str(idx))
    assert (g.n, g.dim) == (n, d)
    q = np.fromfile(qf, dtype=np.float32).reshape(m, d)
    for (comp, ef), (ids, dists, dc) in _read_results(rf, d, m, k, efs).items():
        oids, odists, odc = g.query_k(q, k, ef, bool(comp))
        assert np.array_equal(ids, oids), (comp, ef)
        assert np.array_equal(dists.view(np.uint32), odists.view(np.uint32)), (comp, ef)
        assert np.array_equal(dc.astype(np.uint64), odc), (comp, ef)


@pytest.mark.gpu
def test_reference_sweep_configuration_at_1536(tmp_path, oracle):
    """M = 60, M0 = 120, ef_construction = 480 (the reference's sweep), built by the batched GPU builder:
    bottom-layer lists longer than one wavefront go through the run-time-dim walk, both modes."""
    from expann_amd import AntitopoEngine
    from graph_helpers import check_against_oracle, read_index_degrees
    rng = np.random.RandomState(1536)
    n, d, m, k = 3000, 1536, 48, 10
    base = _sift_like(rng, n, d)
    q = _sift_like(rng, m, d, frac=True)
    idx = str(tmp_path / "c4_1536.index")
    eng = AntitopoEngine(60, 480, 1, 0, False, dim=d)
    eng.store_many_vectors_batched(base, False, 300)
    eng.build()
    eng.save_index(idx)
    engc = AntitopoEngine(60, 480, 1, 0, True, dim=d)
    engc.load_index(idx)
    hdr, deg0 = read_index_degrees(idx)
    assert (hdr["M"], hdr["M0"], hdr["ef_construction"]) == (60, 120, 480)
    assert deg0.max() > 64 and deg0.max() <= 120, deg0.max()
    check_against_oracle(oracle, {False: eng, True: engc}, idx, q, k, efs=(10, 30, 60))
    eng.close()
    engc.close()


@pytest.mark.gpu
def test_compression_needs_a_multiple_of_64(tmp_path):
    from expann_amd import _lib
    L = _lib.load()
    n, d = 64, 48
    vec = np.random.RandomState(48).randint(0, 256, (n, d)).astype(np.float32)
    off = np.arange(n + 1, dtype=np.uint64)
    nb = ((np.arange(n) + 1) % n).astype(np.uint32)
    h = C.c_void_p()
    assert L.expann_graph_create(d, 0, vec.ctypes.data, n, 1, 0, off.ctypes.data, nb.ctypes.data, C.byref(h)) == 0
    q = vec[:2].copy()
    ids = np.zeros((2, 4), np.uint64)
    dists = np.zeros((2, 4), np.float32)
    assert L.expann_graph_search(h, q.ctypes.data, 2, 4, 8, 1, ids.ctypes.data, dists.ctypes.data, None) == 5
    assert b"64" in L.expann_graph_last_error(h)
    assert L.expann_graph_search(h, q.ctypes.data, 2, 4, 8, 0, ids.ctypes.data, dists.ctypes.data, None) == 0
    assert ids[0, 0] == 0 and ids[1, 0] == 1 and dists[0, 0] == 0 and dists[1, 0] == 0
    L.expann_graph_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", [(48, 12000), (1536, 6000)])
def test_batched_builder_at_run_time_dims(tmp_path, oracle, d, n):
    """expann_graph_build_batched through the run-time-dim search and prune kernels: degrees within M / M0, no
    self loops or duplicate edges, edge lengths = oracle.l2_f32 bit for bit, recall within 0.04 of the serial
    graph's, and the GPU walk of the batched graph identical to the oracle's."""
    from graph_helpers import read_index_edges
    M, efc, m, k = 16, 100, 200, 10
    common = ["--n", n, "--m", m, "--d", d, "--k", k, "--M", M, "--ef_construction", efc, "--data", "sift",
              "--build-only", 1]
    idx_b, idx_s, qf = tmp_path / "b.index", tmp_path / "s.index", tmp_path / "q.bin"
    lb = _tool(*common, "--batched", 1024, "--index", idx_b, "--queries", qf)
    assert lb[0]["builder"] == "batched gpu" and lb[0]["batches"] >= 10 and lb[0]["n"] == n
    assert lb[0]["dropped_reverse_edges"] == 0
    hdr, layers = read_index_edges(str(idx_b))
    gb = oracle.Graph(str(idx_b))
    vec = gb.vectors()
    assert vec.shape == (n, d)
    for v, per_layer in enumerate(layers):
        for l, (ids, ds) in enumerate(per_layer):
            assert len(ids) <= (2 * M if l == 0 else M), (v, l, len(ids))
            assert v not in ids and len(set(ids.tolist())) == len(ids)
            assert ids.max(initial=0) < n
    rng = np.random.RandomState(2)
    for v in rng.randint(0, n, 200):
        ids, ds = layers[v][0]
        ref = np.array([oracle.l2_f32(vec[v], vec[j]) for j in ids], dtype=np.float32)
        assert np.array_equal(ref.view(np.uint32), ds.view(np.uint32)), v
    q = np.fromfile(qf, dtype=np.float32).reshape(m, d)
    gt, _ = oracle.brute_force(vec, q, k)
    _tool(*common, "--index", idx_s)
    gs = oracle.Graph(str(idx_s))
    for ef in (10, 60):
        rb = oracle.recall(gb.query_k(q, k, ef)[0], gt)
        rs = oracle.recall(gs.query_k(q, k, ef)[0], gt)
        print(f"d={d} recall@{k} ef={ef}: batched {rb:.4f}, serial {rs:.4f}")
        assert rb > rs - 0.04, (ef, rb, rs)
    # the GPU walk of the batched graph (read back by the tool) against the oracle's
    q2f, rf = tmp_path / "q2.bin", tmp_path / "r.bin"
    _tool("--n", 0, "--m", m, "--d", d, "--k", k, "--read-index", 1, "--index", idx_b, "--queries", q2f,
          "--results", rf, "--ef", 40)
    q2 = np.fromfile(q2f, dtype=np.float32).reshape(m, d)
    for (comp, ef), (ids, dists, dc) in _read_results(rf, d, m, k, [40]).items():
        oids, od, odc = gb.query_k(q2, k, ef, bool(comp))
        assert np.array_equal(ids, oids) and np.array_equal(dists.view(np.uint32), od.view(np.uint32)), comp
        assert np.array_equal(dc.astype(np.uint64), odc), comp


@pytest.mark.gpu
@pytest.mark.parametrize("width,dim", [(1536, 1536), (1000, 1024)])
def test_python_surface_above_960(tmp_path, oracle, width, dim):
    """AntitopoEngine opens rows wider than 960 at the next multiple of 64 (dim chosen from the first rows),
    builds through store_many_vectors_batched, and answers like the oracle on its saved index, fp32 and
    uint8; the other mode's engine loads the same file."""
    from expann_amd import AntitopoEngine
    rng = np.random.RandomState(width)
    base = _sift_like(rng, 2500, width)
    q = _sift_like(rng, 32, width, frac=True)
    built_comp = width != 1536  # (each width builds with a different mode; the other one loads)
    eng = AntitopoEngine(16, 80, 1, 0, built_comp)
    eng.store_many_vectors_batched(base, False, 500)
    assert eng.dim == dim and eng.size() == 2500
    eng.build()
    eng.set_ef_search(40)
    ids, dists = eng.query_many(q, 10)
    idx = tmp_path / "py.index"
    eng.save_index(idx)
    other = AntitopoEngine(16, 80, 1, 0, not built_comp, dim=width)
    assert other.dim == dim
    other.load_index(idx)
    other.set_ef_search(40)
    ids2, dists2 = other.query_many(q, 10)
    g = oracle.Graph(str(idx))
    assert g.dim == dim
    qp = np.zeros((q.shape[0], dim), np.float32)
    qp[:, :width] = q
    for comp, (i, dd) in ((built_comp, (ids, dists)), (not built_comp, (ids2, dists2))):
        oids, od, _ = g.query_k(qp, 10, 40, comp)
        assert np.array_equal(i, oids), comp
        assert np.array_equal(dd.view(np.uint32), od.view(np.uint32)), comp
    assert eng.query_k(q[0], 10) == [int(x) for x in g.query_k(qp[:1], 10, 40, built_comp)[0][0]]
    with pytest.raises(ValueError, match="4096"):
        AntitopoEngine(16, 80, 1, 0, False, dim=4160)
    eng.close()
    other.close()


@pytest.mark.gpu
def test_row_offsets_past_2_to_the_32(tmp_path):
    """1.05 M rows x 4096: the element offset of a row above 2^20 passes 2^32 (fp32 and the uint8 copy).  A
    hand-made graph -- layer 0 a ring plus random chords, layer 1 the starting vertex linked to the targets
    -- and queries that are copies of target rows: the walk must return each target at distance 0."""
    from expann_amd import _lib
    L = _lib.load()
    n, d, m, k = 1_050_000, 4096, 64, 10
    rng = np.random.RandomState(4096)
    vec = np.empty((n, d), np.float32)
    vec[:] = rng.randint(0, 200, d).astype(np.float32)
    rows = np.arange(n)
    for b in range(3):  # rows differ in their first three bytes (the uint8 copy as well)
        vec[:, b] = ((rows >> (8 * b)) & 255).astype(np.float32)
    targets = np.sort(rng.choice(np.arange((1 << 20) + 1, n), m, replace=False)).astype(np.uint32)
    assert (targets.astype(np.uint64) * d >= (1 << 32)).all()
    # layer 0: i -> i + 1, i - 1 and two random chords
    nb0 = np.stack([(rows + 1) % n, (rows - 1) % n, rng.randint(0, n, n), rng.randint(0, n, n)], axis=1)
    nb0 = nb0.astype(np.uint32).ravel()
    deg1 = np.zeros(n, np.uint64)
    deg1[0] = m
    deg1[targets] = 1
    off = np.zeros((2, n + 1), np.uint64)
    off[0] = np.arange(n + 1, dtype=np.uint64) * 4
    off[1, 0] = 4 * n
    off[1, 1:] = 4 * n + np.cumsum(deg1)
    nb1 = np.empty(int(deg1.sum()), np.uint32)
    nb1[:m] = targets                       # vertex 0's layer-1 list
    nb1[m:] = 0                             # each target's: vertex 0
    nb = np.concatenate([nb0, nb1])
    h = C.c_void_p()
    rc = L.expann_graph_create(d, 0, vec.ctypes.data, n, 2, 0, off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    q = np.ascontiguousarray(vec[targets])
    del vec
    ids = np.zeros((m, k), np.uint64)
    dists = np.zeros((m, k), np.float32)
    for comp in (0, 1):
        rc = L.expann_graph_search(h, q.ctypes.data, m, k, 16, comp, ids.ctypes.data, dists.ctypes.data, None)
        assert rc == 0, L.expann_graph_last_error(h)
        assert np.array_equal(ids[:, 0], targets.astype(np.uint64)), comp
        assert (dists[:, 0] == 0).all() and (dists[:, 1] > 0).all(), comp
    L.expann_graph_destroy(h)
