"""AntitopoEngine.append (THE GRAPH APPEND RULE, include/expann_hip.h) on the GPU.

An appended engine is compared with its TWIN: a second engine given the same rows by
store_many_vectors_batched(base), store_many_vectors_batched(new) ..., build() -- the route every engine took
before.  The two saved index files must agree in size, max_layer, starting_vertex and in every (vertex, layer) row
as a sorted list of (distance bits, id) (graph_append_helpers.py), without tolerances.  Rows are Gaussian: distance
ties are the only way the order of rows can leak into a multi-batch build (tests/test_gpu_graph_build_exact.py).
The device graph is compared with the host graph through the oracle's walk over the saved file, bit for bit.

The level draws are one fixed sequence (mt19937(0), one draw per vertex, whatever the rows are): under it no M opens
a layer between vertex 220 and vertex 7546, so the test that needs a new layer appends 1 500 rows to 7 000."""
import ctypes as C

import numpy as np
import pytest

from graph_append_helpers import assert_same_index, read_index

pytestmark = pytest.mark.gpu
PAD = np.uint64(2 ** 64 - 1)
N_SERIAL = 500  # rows of an empty engine that go through the serial host builder


def _gauss(seed, n, d):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def _engine(base, M, efc, ortho_count=1, rows="f32", comp=False, n_serial=N_SERIAL):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M, efc, ortho_count, 0, comp, dim=base.shape[1], rows=rows)
    eng.store_many_vectors_batched(base, False, n_serial)
    eng.build()
    return eng


def _twin_index(path, base, news, M, efc, **kw):
    """the saved index of the engine that stored base as _engine does and every block of `news` by
    store_many_vectors_batched with its default n_serial -- the rule's store_rows_batched(rows, n) -- then built"""
    from expann_amd import AntitopoEngine
    n_serial = kw.pop("n_serial", N_SERIAL)
    eng = AntitopoEngine(M, efc, kw.pop("ortho_count", 1), 0, False, dim=base.shape[1], **kw)
    eng.store_many_vectors_batched(base, False, n_serial)
    for new in news:
        eng.store_many_vectors_batched(new, False)
    eng.build()
    eng.save_index(path)
    return eng


def _stats(eng, *names):
    return tuple(eng.stat(n) for n in names)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _oracle_equal(oracle, eng, path, q, k, ef, comp=False):
    """eng.query_many == the oracle's walk over the index file: ids, distance bits, distcomps"""
    eng.set_ef_search(ef)
    before = int(eng.param_list()["num_distcomps"])
    ids, dists = eng.query_many(q, k)
    oids, od, odc = oracle.Graph(str(path)).query_k(q, k, ef, comp)
    assert np.array_equal(ids, oids)
    assert np.array_equal(_bits(dists), _bits(od))
    assert int(eng.param_list()["num_distcomps"]) - before == int(odc.sum())


def test_one_batch_equals_the_twin(tmp_path):
    base, new = _gauss(1, 3000, 64), _gauss(2, 150, 64)
    eng = _engine(base, 16, 80)
    assert _stats(eng, "append_calls", "capacity_rows") == (0, 3000)
    assert eng.append(new) == 150 and eng.size() == 3150
    assert _stats(eng, "append_calls", "append_rows", "append_device", "append_batches", "append_host") == (1, 150, 1, 1, 0)
    eng.save_index(tmp_path / "a.index")
    _twin_index(tmp_path / "t.index", base, [new], 16, 80).close()
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    eng.close()


@pytest.fixture(scope="module")
def grown(tmp_path_factory):
    """7 000 rows plus 1 500 at M = 12: many batches, vertex 7546 opens layer 4; the engine stays open, its index and
    its twin's are saved"""
    tmp = tmp_path_factory.mktemp("graph_append")
    base, new = _gauss(3, 7000, 64), _gauss(4, 1500, 64)
    eng = _engine(base, 12, 60)
    eng.save_index(tmp / "before.index")
    assert eng.append(new) == 1500
    stats = _stats(eng, "append_batches", "append_device", "append_host")
    eng.save_index(tmp / "after.index")
    _twin_index(tmp / "twin.index", base, [new], 12, 60).close()
    yield dict(eng=eng, tmp=tmp, base=base, new=new, stats=stats, q=_gauss(5, 32, 64))
    eng.close()


def test_many_batches_new_upper_vertices_and_a_new_layer(grown):
    tmp = grown["tmp"]
    before = read_index(tmp / "before.index")
    after = assert_same_index(tmp / "after.index", tmp / "twin.index")
    assert after["size"] == 8500 and grown["eng"].size() == 8500
    assert after["max_layer"] > before["max_layer"]  # a layer was opened ...
    assert after["starting_vertex"] >= 7000          # ... by an appended vertex
    assert (after["levels"] >= 1).sum() > (before["levels"] >= 1).sum() + 50  # and the upper layers grew
    batches, device, host = grown["stats"]
    assert batches >= 4 and device == 1 and host == 0
    assert grown["eng"].stat("append_edges") == after["edges"]  # what the device's scan counted
    # the rows before the append kept their vectors and their levels
    assert np.array_equal(after["levels"][:7000], before["levels"])


@pytest.mark.parametrize("ef", [10, 40])
def test_the_device_graph_is_the_host_graph_fp32(grown, oracle, ef):
    _oracle_equal(oracle, grown["eng"], grown["tmp"] / "after.index", grown["q"], 10, ef)


def test_the_device_graph_is_the_host_graph_ranged_range_and_filter(grown):
    """the ranged walk and the range search answer as a fresh engine that loads the saved index (the oracle walks fp32
    and the uint8 cast only); a filter set after the append that allows only appended rows returns only those"""
    from expann_amd import AntitopoEngine
    eng, q = grown["eng"], grown["q"]
    fresh = AntitopoEngine(12, 60, 1, 0, False, dim=64)
    fresh.load_index(grown["tmp"] / "after.index")
    for e in (eng, fresh):
        e.set_ef_search(40)
    radius = float(np.sort(((grown["base"][:2000] - q[0]) ** 2).sum(1))[20])
    a, b = eng.range_search(q, radius, 32), fresh.range_search(q, radius, 32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])
    assert a[2].max() > 0
    for e in (eng, fresh):
        e.set_compression("ranged")
    a, b = eng.query_many(q, 10), fresh.query_many(q, 10)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
    eng.set_compression("none")
    fresh.close()
    allow = np.zeros(8500, bool)
    allow[7000:] = True
    eng.set_row_filter(allow)
    assert eng.stat("filter_active") == 1 and eng.stat("filter_rows") == 1500
    ids, _ = eng.query_many(q, 10)
    assert (ids != PAD).sum() >= 5 * len(q) and (ids[ids != PAD] >= 7000).all()
    eng.set_row_filter(None)


def test_the_uint8_walk_after_an_append(tmp_path, oracle):
    """integer-valued rows at d = 64 (ties: no twin here), fp32 and the uint8 cast against the oracle on the saved index"""
    rng = np.random.RandomState(6)
    rows = np.clip(np.round(np.abs(rng.standard_normal((3300, 64))) * 40.0), 0, 255).astype(np.float32)
    q = (rows[rng.choice(3300, 32)] + rng.uniform(0, 0.99, (32, 64))).astype(np.float32)
    eng = _engine(rows[:3000], 16, 80, comp=True)
    eng.set_ef_search(40)
    eng.query_many(q, 10)  # (the uint8 copy of 3 000 rows exists: the append must drop it)
    assert eng.append(rows[3000:]) == 300 and eng.stat("append_device") == 1
    eng.save_index(tmp_path / "u8.index")
    _oracle_equal(oracle, eng, tmp_path / "u8.index", q, 10, 40, comp=True)
    eng.set_compression("none")
    _oracle_equal(oracle, eng, tmp_path / "u8.index", q, 10, 40, comp=False)
    eng.close()


def test_two_appends_then_save_then_a_serial_store(tmp_path):
    base, n1, n2, extra = _gauss(7, 2500, 64), _gauss(8, 120, 64), _gauss(9, 200, 64), _gauss(10, 20, 64)
    eng = _engine(base, 10, 50)
    assert eng.append(n1) == 120 and eng.append(n2) == 200  # nothing reads the host graph in between
    assert eng.size() == 2820 and _stats(eng, "append_calls", "append_rows", "append_device") == (2, 320, 2)
    eng.save_index(tmp_path / "a.index")
    twin = _twin_index(tmp_path / "t.index", base, [n1, n2], 10, 50)
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    for e, name in ((eng, "a2.index"), (twin, "t2.index")):
        e.store_many_vectors(extra, False)
        e.build()
        e.save_index(tmp_path / name)
        e.close()
    assert_same_index(tmp_path / "a2.index", tmp_path / "t2.index")


def test_a_full_handle_grows_by_half(tmp_path):
    base, n1, n2 = _gauss(11, 3000, 64), _gauss(12, 150, 64), _gauss(13, 1400, 64)
    eng = _engine(base, 8, 40)
    assert eng.append(n1) == 150
    assert _stats(eng, "graph_reallocs", "capacity_rows") == (1, 4500)
    assert eng.append(n2) == 1400  # 4 550 rows: past the capacity again
    assert _stats(eng, "graph_reallocs", "capacity_rows") == (2, 6750)
    eng.save_index(tmp_path / "a.index")
    _twin_index(tmp_path / "t.index", base, [n1, n2], 8, 40).close()
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    eng.close()


def test_reserve_then_appends_reallocate_nothing(tmp_path, oracle):
    base, n1, n2 = _gauss(14, 3000, 64), _gauss(15, 150, 64), _gauss(16, 150, 64)
    eng = _engine(base, 16, 60)
    eng.reserve(100)  # below the size: nothing happens
    assert eng.stat("capacity_rows") == 3000
    eng.reserve(3300)
    assert _stats(eng, "capacity_rows", "graph_reallocs") == (3300, 0)
    eng.set_ef_search(20)
    q = _gauss(17, 16, 64)
    before = eng.query_many(q, 10)
    assert eng.append(n1) == 150 and eng.append(n2) == 150
    assert _stats(eng, "capacity_rows", "graph_reallocs", "append_device") == (3300, 0, 2)
    eng.save_index(tmp_path / "a.index")
    _twin_index(tmp_path / "t.index", base, [n1, n2], 16, 60).close()
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    _oracle_equal(oracle, eng, tmp_path / "a.index", q, 10, 20)
    assert before[0].shape == (16, 10)
    eng.close()


def test_across_a_multiple_of_8192_rows(tmp_path, oracle):
    """8 100 rows plus 200: the visited bitsets' word count changes with the capacity"""
    base, new = _gauss(18, 8100, 64), _gauss(19, 200, 64)
    eng = _engine(base, 12, 40)
    assert eng.append(new) == 200 and eng.size() == 8300
    eng.save_index(tmp_path / "a.index")
    for ef in (10, 50):
        _oracle_equal(oracle, eng, tmp_path / "a.index", _gauss(20, 32, 64), 10, ef)
    ids, dists = eng.query_many(new[:16], 1)
    assert np.array_equal(ids[:, 0], np.arange(8100, 8116, dtype=np.uint64)) and (dists == 0).all()
    eng.close()


def test_run_time_dim_instances(tmp_path, oracle):
    """d = 80 through the C ABI (the Python surface would pad the rows to 128, a compiled dim)"""
    base, new = _gauss(21, 2600, 80), _gauss(22, 300, 80)
    from expann_amd import _lib
    L = _lib.load()

    def make(blocks):
        h = C.c_void_p()
        assert L.expann_antitopo_create(80, 0, 14, 60, 1, 0, 0, C.byref(h)) == 0
        for b in blocks:
            assert L.expann_antitopo_store_batched(h, b.ctypes.data, len(b), N_SERIAL) == 0
        assert L.expann_antitopo_build(h) == 0
        return h
    h, twin = make([base]), make([base, new])
    done = C.c_size_t(0)
    assert L.expann_antitopo_append(h, new.ctypes.data, len(new), C.byref(done)) == 0, L.expann_antitopo_last_error(h)
    assert done.value == 300 and L.expann_antitopo_size(h) == 2900
    out = C.c_uint64(0)
    assert L.expann_antitopo_get_stat(h, b"append_device", C.byref(out)) == 0 and out.value == 1
    assert L.expann_antitopo_save(h, str(tmp_path / "a.index").encode()) == 0
    assert L.expann_antitopo_save(twin, str(tmp_path / "t.index").encode()) == 0
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    q = _gauss(23, 32, 80)
    ids, dists = np.empty((32, 10), np.uint64), np.empty((32, 10), np.float32)
    assert L.expann_antitopo_set_ef_search(h, 30) == 0
    assert L.expann_antitopo_query(h, q.ctypes.data, 32, 10, ids.ctypes.data, dists.ctypes.data) == 0
    oids, od, odc = oracle.Graph(str(tmp_path / "a.index")).query_k(q, 10, 30, False)
    assert np.array_equal(ids, oids) and np.array_equal(_bits(dists), _bits(od))
    assert L.expann_antitopo_num_distcomps(h) == int(odc.sum())
    L.expann_antitopo_destroy(h)
    L.expann_antitopo_destroy(twin)


def test_an_append_waits_for_the_device_buffer_searches():
    import torch
    base, new = _gauss(24, 3000, 64), _gauss(25, 100, 64)
    eng = _engine(base, 16, 60)
    eng.set_ef_search(40)
    q = _gauss(26, 64, 64)
    want_ids, want_d = eng.query_many(q, 10)  # the graph before the append
    tq = torch.from_numpy(q).cuda()
    ids = torch.full((64, 10), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((64, 10), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.query_many_device(tq.data_ptr(), 64, 10, ids.data_ptr(), dists.data_ptr())
    assert eng.append(new) == 100  # no sync in between
    eng.sync()
    assert np.array_equal(ids.cpu().numpy().view(np.uint64), want_ids)
    assert np.array_equal(_bits(dists.cpu().numpy()), _bits(want_d))
    got, d = eng.query_many(new[:32], 1)
    assert np.array_equal(got[:, 0], np.arange(3000, 3032, dtype=np.uint64)) and (d == 0).all()
    eng.close()


def test_filter_and_groups_are_cleared():
    base, new = _gauss(27, 2400, 64), _gauss(28, 64, 64)
    eng = _engine(base, 16, 40)
    eng.set_row_filter(np.arange(2400) % 2 == 0)
    eng.set_row_groups(np.arange(2400, dtype=np.uint32) % 7)
    assert _stats(eng, "filter_active", "groups_active") == (1, 1)
    assert eng.append(new) == 64
    assert _stats(eng, "filter_active", "groups_active", "filter_rows", "append_device") == (0, 0, 2464, 1)
    eng.close()


@pytest.mark.parametrize("case", ["f16", "ortho2", "small"])
def test_the_host_route(tmp_path, case):
    kw, n, M, efc = {}, 1000, 12, 40
    if case == "f16":
        kw, n = dict(rows="f16"), 2500
    elif case == "ortho2":
        kw, n = dict(ortho_count=2), 300
    base, new = _gauss(29, n, 64), _gauss(30, 60, 64)
    eng = _engine(base, M, efc, **kw)
    eng.reserve(n + 500)  # (an engine of the host route keeps no capacity)
    assert eng.append(new) == 60 and eng.size() == n + 60
    assert _stats(eng, "append_calls", "append_rows", "append_host", "append_device", "append_batches") == (1, 60, 1, 0, 0)
    assert eng.append(new[:7]) == 7
    assert _stats(eng, "append_calls", "append_rows", "append_host", "append_device") == (2, 67, 2, 0)
    eng.save_index(tmp_path / "a.index")
    _twin_index(tmp_path / "t.index", base, [new, new[:7]], M, efc, **kw).close()
    assert_same_index(tmp_path / "a.index", tmp_path / "t.index")
    eng.close()


def test_argument_checks_with_a_handle():
    from expann_amd import AntitopoEngine, _lib
    L = _lib.load()
    eng = AntitopoEngine(16, 40, 1, 0, False, dim=64)  # opened, not built
    row = np.zeros((1, 64), np.float32)
    done = C.c_size_t(7)
    assert L.expann_antitopo_append(eng._h, row.ctypes.data, 1, C.byref(done)) == _lib.ERR_NOT_BUILT and done.value == 0
    assert L.expann_antitopo_append(eng._h, None, 1, None) == _lib.ERR_INVALID_ARG
    assert L.expann_antitopo_reserve(eng._h, 10) == _lib.ERR_NOT_BUILT
    out = C.c_uint64(0)
    assert L.expann_antitopo_get_stat(eng._h, b"append_calls", C.byref(out)) == _lib.ERR_NOT_BUILT
    eng.store_many_vectors_batched(_gauss(31, 2100, 64), False, N_SERIAL)
    eng.build()
    assert L.expann_antitopo_append(eng._h, None, 0, None) == 0  # n == 0: nothing happens
    assert eng.append(np.zeros((0, 64), np.float32)) == 0
    assert L.expann_antitopo_append(eng._h, None, 1, C.byref(done)) == _lib.ERR_INVALID_ARG
    assert _stats(eng, "append_calls", "append_rows", "capacity_rows") == (0, 0, 2100) and eng.size() == 2100
    assert L.expann_antitopo_get_stat(eng._h, b"no_such_stat", C.byref(out)) == _lib.ERR_INVALID_ARG
    eng.close()


def test_cpp_engine_append_rows():
    """gpu_antitopo_engine<float>::append_rows / reserve against its twin (expann_amd/host/expann_graph_append_check.cpp)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "expann_amd", "host", "expann_graph_append_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout
