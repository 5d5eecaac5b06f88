"""AntitopoEngine.remove / compact_row_filter (THE GRAPH REMOVE RULE, include/expann_hip.h) on the GPU.

Every case saves the engine before and after the call and compares the second file with the NumPy restatement of the
rule (tests/graph_remove_helpers.py) applied to the first: header, rows, every edge and every length bit, no
tolerances.  The device graph is then compared with a fresh engine that loads the saved file -- query_many,
query_many_device, grouped and range searches: ids, distance bits, counts -- and the plain walk with the oracle's walk
over that file, distance evaluations included.

Rows are Gaussian, d = 64, M = 16 (M0 = 32), ef_construction = 80, 3 000 rows built with
store_many_vectors_batched(..., 500): above the 2 048 rows of the host route, the settings of the append's tests."""
import ctypes as C
import os

import numpy as np
import pytest

import graph_remove_helpers as grh
from graph_helpers import read_index_edges

pytestmark = pytest.mark.gpu
PAD = np.uint64(2 ** 64 - 1)
N_SERIAL = 500
REMOVE_STATS = ("remove_calls", "remove_rows", "remove_touched_rows", "remove_truncated_rows", "remove_device",
                "remove_host")
# repaired recall@10 >= fresh recall@10 - RECALL_MARGIN at 30 % removed.  Measured over the data seeds 0 .. 9
# (recall_pair below; the ten pairs stand in DESIGN.md 4.9l): the largest gap fresh - repaired was 0.0542 (seed 8:
# 0.9000 against 0.9542), the smallest 0.0208; the margin is twice the largest, for the seeds not tried.
RECALL_MARGIN = 2 * 0.0542


def _gauss(seed, n, d=64):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def _engine(base, M=16, efc=80, po=0, ortho_count=1, rows="f32", n_serial=N_SERIAL):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M, efc, ortho_count, po, False, dim=base.shape[1], rows=rows)
    eng.store_many_vectors_batched(base, False, n_serial)
    eng.build()
    return eng


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)


def _device_query(eng, q, k, groups=None):
    import torch
    tq = torch.from_numpy(q).cuda()
    ids = torch.full((len(q), k), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((len(q), k), -1.0, dtype=torch.float32, device="cuda")
    tg = torch.from_numpy(groups.astype(np.int32)).cuda() if groups is not None else None
    torch.cuda.synchronize()
    eng.query_many_device(tq.data_ptr(), len(q), k, ids.data_ptr(), dists.data_ptr(),
                          groups_ptr=tg.data_ptr() if tg is not None else 0)
    eng.sync()
    return ids.cpu().numpy().view(np.uint64), dists.cpu().numpy()


def _answers_as_a_fresh_engine(eng, path, q, oracle, M, efc, po=0, ef=40, **kw):
    """every search entry point of `eng` == a fresh engine that loaded `path`; the plain walk == the oracle's"""
    from expann_amd import AntitopoEngine
    fresh = AntitopoEngine(M, efc, kw.get("ortho_count", 1), po, False, dim=q.shape[1], rows=kw.get("rows", "f32"))
    fresh.load_index(path)
    n = eng.size()
    assert fresh.size() == n
    labels = (np.arange(n) % 5).astype(np.uint32)
    qg = (np.arange(len(q)) % 5).astype(np.uint32)
    base = grh.read_index_rows(str(path))[0]
    radius = float(np.sort(((base - q[0]) ** 2).sum(1))[min(20, n - 1)])
    got = []
    for e in (eng, fresh):
        e.set_ef_search(ef)
        before = int(e.param_list()["num_distcomps"])
        plain = e.query_many(q, 10)
        evals = int(e.param_list()["num_distcomps"]) - before
        out = [*plain, np.array([evals]), *_device_query(e, q, 10)]
        e.set_row_groups(labels)
        out += [*e.query_many(q, 10, groups=qg), *_device_query(e, q, 10, qg)]
        e.set_row_groups(None)
        out += [*e.range_search(q, radius, 32)]
        got.append(out)
    fresh.close()
    _same(got[0], got[1])
    ids, dists, evals = got[0][:3]
    oids, od, odc = oracle.Graph(str(path)).query_k(q, 10, ef, False)
    assert np.array_equal(ids, oids) and np.array_equal(_bits(dists), _bits(od)) and int(evals[0]) == int(odc.sum())
    assert np.array_equal(got[0][3], ids) and np.array_equal(_bits(got[0][4]), _bits(dists))  # device buffers == host buffers
    assert got[0][-1].max() > 0
    return ids


def _remove_and_check(eng, tmp, ids, oracle, q, M=16, efc=80, po=0, tag="r", device=True, **kw):
    """save, remove, save; the second file == the restatement of the first; the device graph == the second file.
    Returns the restatement."""
    before, after = tmp / f"{tag}_before.index", tmp / f"{tag}_after.index"
    eng.save_index(before)
    n, stats = eng.size(), [eng.stat(s) for s in REMOVE_STATS]
    ids = np.asarray(ids, np.uint64)
    distinct = len(np.unique(ids))
    assert eng.remove(ids) == distinct and eng.size() == n - distinct
    eng.save_index(after)
    want = grh.apply_remove(str(before), ids)
    grh.assert_file_is(str(after), want)
    now = [eng.stat(s) for s in REMOVE_STATS]
    assert now[0] == stats[0] + 1 and now[1] == stats[1] + distinct
    if device:
        assert now[2:] == [stats[2] + want["touched"], stats[3] + want["truncated"], stats[4] + 1, stats[5]]
        assert want["touched"] == 0 or eng.stat("remove_repair_ns") > 0
    else:
        assert (now[4], now[5]) == (stats[4], stats[5] + 1)
    _answers_as_a_fresh_engine(eng, after, q, oracle, M, efc, po, **kw)
    return want


@pytest.fixture(scope="module")
def queries():
    return _gauss(99, 32)


def test_random_ids_unordered_with_repeats(tmp_path, oracle, queries):
    eng = _engine(_gauss(1, 3000))
    rng = np.random.RandomState(2)
    ids = rng.choice(3000, 300, replace=False)
    ids = np.concatenate([ids, ids[:25]])
    rng.shuffle(ids)
    want = _remove_and_check(eng, tmp_path, ids, oracle, queries)
    assert want["touched"] > 1000 and eng.stat("capacity_rows") == 3000
    eng.close()


def test_most_of_one_row_is_removed_and_the_candidates_are_truncated(tmp_path, oracle, queries):
    eng = _engine(_gauss(3, 3000))
    eng.save_index(tmp_path / "g.index")
    _, layers = read_index_edges(str(tmp_path / "g.index"))
    v = next(v for v in range(3000) if len(layers[v][0][0]) == 32)
    want = _remove_and_check(eng, tmp_path, layers[v][0][0][:24], oracle, queries)
    assert want["truncated"] > 0 and eng.stat("remove_truncated_rows") == want["truncated"]
    eng.close()


def test_a_two_hop_neighbourhood_leaves_an_empty_row_that_the_walk_survives(tmp_path, oracle, queries):
    base = _gauss(4, 3000)
    eng = _engine(base)
    eng.save_index(tmp_path / "g.index")
    _, layers = read_index_edges(str(tmp_path / "g.index"))
    v = next(v for v in range(100, 3000) if len(layers[v]) == 1 and len(layers[v][0][0]) > 0)
    hood = set()
    for a in layers[v][0][0]:
        hood.add(int(a))
        hood.update(int(b) for b in layers[int(a)][0][0])
    hood.discard(v)
    want = _remove_and_check(eng, tmp_path, sorted(hood), oracle, queries)
    new_v = v - sum(1 for s in hood if s < v)
    assert want["empty_rows"] > 0 and len(want["layers"][new_v][0][0]) == 0
    ids, dists = eng.query_many(base[v:v + 1], 10)  # the walk does not reach a vertex nobody points to ... and survives
    assert (ids != PAD).all()
    eng.close()


def test_the_top_of_the_graph_is_removed_and_max_layer_drops(tmp_path, oracle, queries):
    eng = _engine(_gauss(5, 3000))
    eng.save_index(tmp_path / "g.index")
    hdr, layers = read_index_edges(str(tmp_path / "g.index"))
    assert hdr["max_layer"] >= 3
    ids = [hdr["starting_vertex"]] + [v for v in range(3000) if len(layers[v]) >= 3]
    want = _remove_and_check(eng, tmp_path, ids, oracle, queries)
    assert want["max_layer"] == 2 < hdr["max_layer"]
    eng.close()


def test_duplicate_rows_and_prune_overflow(tmp_path, oracle, queries):
    """5 % exact duplicates: zero lengths and ties in (length, id) order"""
    base = _gauss(6, 3000)
    rng = np.random.RandomState(7)
    dup = rng.choice(3000, 150, replace=False)
    base[dup] = base[(dup + 1 + rng.randint(0, 2000, 150)) % 3000]
    eng = _engine(base, po=1)
    ids = np.concatenate([rng.choice(3000, 250, replace=False), dup[:40]])
    _remove_and_check(eng, tmp_path, ids, oracle, queries, po=1)
    eng.close()


def test_run_time_dim_instances(tmp_path, oracle):
    """d = 80 through the C ABI (the Python surface would pad the rows to 128, a compiled dim): the D = 0 prune"""
    from expann_amd import _lib
    L = _lib.load()
    base = _gauss(8, 2600, 80)
    h = C.c_void_p()
    assert L.expann_antitopo_create(80, 0, 14, 60, 1, 0, 0, C.byref(h)) == 0
    assert L.expann_antitopo_store_batched(h, base.ctypes.data, len(base), N_SERIAL) == 0
    assert L.expann_antitopo_build(h) == 0
    before, after = str(tmp_path / "b.index"), str(tmp_path / "a.index")
    assert L.expann_antitopo_save(h, before.encode()) == 0
    ids = np.random.RandomState(9).choice(2600, 260, replace=False).astype(np.uint64)
    done = C.c_size_t(0)
    assert L.expann_antitopo_remove(h, ids.ctypes.data, len(ids), C.byref(done)) == 0, L.expann_antitopo_last_error(h)
    assert done.value == 260 and L.expann_antitopo_size(h) == 2340
    out = C.c_uint64(0)
    assert L.expann_antitopo_get_stat(h, b"remove_device", C.byref(out)) == 0 and out.value == 1
    assert L.expann_antitopo_save(h, after.encode()) == 0
    grh.assert_file_is(after, grh.apply_remove(before, ids))
    q = _gauss(10, 32, 80)
    got, dists = np.empty((32, 10), np.uint64), np.empty((32, 10), np.float32)
    assert L.expann_antitopo_set_ef_search(h, 30) == 0
    assert L.expann_antitopo_query(h, q.ctypes.data, 32, 10, got.ctypes.data, dists.ctypes.data) == 0
    oids, od, odc = oracle.Graph(after).query_k(q, 10, 30, False)
    assert np.array_equal(got, oids) and np.array_equal(_bits(dists), _bits(od))
    assert L.expann_antitopo_num_distcomps(h) == int(odc.sum())
    L.expann_antitopo_destroy(h)


def test_across_a_multiple_of_8192_rows(tmp_path, oracle, queries):
    eng = _engine(_gauss(11, 8300), M=8, efc=40)
    ids = np.random.RandomState(12).choice(8300, 200, replace=False)
    _remove_and_check(eng, tmp_path, ids, oracle, queries, M=8, efc=40)
    assert eng.size() == 8100 and eng.stat("capacity_rows") == 8300
    eng.close()


def test_remove_append_remove_append_with_a_reserve(tmp_path, oracle, queries):
    from graph_append_helpers import read_index
    base, n1, n2 = _gauss(13, 3000), _gauss(14, 200), _gauss(15, 120)
    eng = _engine(base)
    eng.reserve(3400)
    rng = np.random.RandomState(16)
    _remove_and_check(eng, tmp_path, rng.choice(3000, 150, replace=False), oracle, queries, tag="a")
    assert eng.append(n1) == 200 and eng.size() == 3050
    got, d = eng.query_many(n1[:16], 1)
    assert np.array_equal(got[:, 0], np.arange(2850, 2866, dtype=np.uint64)) and (d == 0).all()
    _remove_and_check(eng, tmp_path, rng.choice(3050, 100, replace=False), oracle, queries, tag="b")
    assert eng.append(n2) == 120 and eng.size() == 3070
    got, d = eng.query_many(n2[:16], 1)
    assert np.array_equal(got[:, 0], np.arange(2950, 2966, dtype=np.uint64)) and (d == 0).all()
    assert (eng.stat("capacity_rows"), eng.stat("graph_reallocs"), eng.stat("remove_device"), eng.stat("append_device")) == \
        (3400, 0, 2, 2)
    # the level generator went on as if nothing had been removed: the last rows have the levels of draws 3201 .. 3320
    eng.save_index(tmp_path / "end.index")
    twin = _engine(np.concatenate([base, n1, n2]))
    twin.save_index(tmp_path / "twin.index")
    twin.close()
    assert np.array_equal(read_index(tmp_path / "end.index")["levels"][-120:], read_index(tmp_path / "twin.index")["levels"][-120:])
    _answers_as_a_fresh_engine(eng, tmp_path / "end.index", queries, oracle, 16, 80)
    eng.close()


def test_a_remove_waits_for_the_device_buffer_searches():
    import torch
    eng = _engine(_gauss(17, 3000))
    eng.set_ef_search(40)
    q = _gauss(18, 64)
    want_ids, want_d = eng.query_many(q, 10)  # the graph before the remove
    tq = torch.from_numpy(q).cuda()
    ids = torch.full((64, 10), -2, dtype=torch.int64, device="cuda")
    dists = torch.full((64, 10), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.query_many_device(tq.data_ptr(), 64, 10, ids.data_ptr(), dists.data_ptr())
    gone = np.unique(want_ids[:, 0])
    assert eng.remove(gone) == len(gone)  # no sync in between
    eng.sync()
    assert np.array_equal(ids.cpu().numpy().view(np.uint64), want_ids)
    assert np.array_equal(_bits(dists.cpu().numpy()), _bits(want_d))
    now, _ = eng.query_many(q, 10)
    assert not np.array_equal(now, want_ids)
    eng.close()


def test_filter_and_groups_are_cleared():
    eng = _engine(_gauss(19, 2400), efc=40)
    eng.set_row_filter(np.arange(2400) % 2 == 0)
    eng.set_row_groups(np.arange(2400, dtype=np.uint32) % 7)
    assert (eng.stat("filter_active"), eng.stat("groups_active")) == (1, 1)
    assert eng.remove([5, 17, 2399]) == 3
    assert (eng.stat("filter_active"), eng.stat("groups_active"), eng.stat("filter_rows"), eng.stat("remove_device")) == \
        (0, 0, 2397, 1)
    eng.close()


def test_compact_row_filter_is_remove_of_the_disallowed_rows(tmp_path):
    from expann_amd import _lib
    base = _gauss(20, 3000)
    allow = np.random.RandomState(21).rand(3000) < 0.5
    a, b = _engine(base), _engine(base)
    with pytest.raises(_lib.ExpannError) as ei:  # no filter in force
        a.compact_row_filter()
    assert ei.value.code == _lib.ERR_INVALID_ARG
    a.set_row_filter(np.zeros(3000, bool))
    with pytest.raises(_lib.ExpannError) as ei:  # a filter that allows no row
        a.compact_row_filter()
    assert ei.value.code == _lib.ERR_INVALID_ARG and a.size() == 3000 and a.stat("filter_active") == 1
    a.set_row_filter(np.ones(3000, bool))
    assert a.compact_row_filter() == 0 and a.stat("filter_active") == 0 and a.stat("remove_calls") == 0
    a.set_row_filter(allow)
    assert a.compact_row_filter() == int((~allow).sum()) and a.stat("filter_active") == 0
    assert b.remove(np.nonzero(~allow)[0]) == int((~allow).sum())
    a.save_index(tmp_path / "a.index")
    b.save_index(tmp_path / "b.index")
    assert open(tmp_path / "a.index", "rb").read() == open(tmp_path / "b.index", "rb").read()
    a.close()
    b.close()


@pytest.mark.parametrize("case", ["f16", "ortho2", "small"])
def test_the_host_route(tmp_path, oracle, queries, case):
    kw, n, M, efc = {}, 1500, 12, 40
    if case == "f16":
        kw, n = dict(rows="f16"), 2500
    elif case == "ortho2":
        kw, n = dict(ortho_count=2), 300
    eng = _engine(_gauss(22, n), M, efc, **kw)
    rng = np.random.RandomState(23)
    ids = rng.choice(n, n // 10, replace=False)
    _remove_and_check(eng, tmp_path, np.concatenate([ids, ids[:5]]), oracle, queries, M, efc, tag="h1", device=False, **kw)
    _remove_and_check(eng, tmp_path, rng.choice(n - n // 10, 7, replace=False), oracle, queries, M, efc, tag="h2",
                      device=False, **kw)
    assert (eng.stat("remove_calls"), eng.stat("remove_rows"), eng.stat("remove_host")) == (2, n // 10 + 7, 2)
    eng.close()


def test_refusals_leave_the_engine_as_it_was(tmp_path, queries):
    from expann_amd import AntitopoEngine, _lib
    L = _lib.load()
    opened = AntitopoEngine(16, 40, 1, 0, False, dim=64)  # opened, not built
    one = np.array([1], np.uint64)
    done = C.c_size_t(7)
    assert L.expann_antitopo_remove(opened._h, one.ctypes.data, 1, C.byref(done)) == _lib.ERR_NOT_BUILT and done.value == 0
    assert L.expann_antitopo_compact_row_filter(opened._h, None) == _lib.ERR_NOT_BUILT
    opened.close()
    eng = _engine(_gauss(24, 2500), efc=40)
    eng.set_ef_search(30)
    assert eng.remove([3, 9]) == 2  # (the builder's state is resident from here on: the device route refuses too)
    eng.save_index(tmp_path / "1.index")
    want = eng.query_many(queries, 10)
    for bad in ([4, 2498], np.arange(2498), [2 ** 40]):
        with pytest.raises(_lib.ExpannError) as ei:
            eng.remove(bad)
        assert ei.value.code == _lib.ERR_INVALID_ARG
    assert L.expann_antitopo_remove(eng._h, None, 1, C.byref(done)) == _lib.ERR_INVALID_ARG and done.value == 0
    assert L.expann_antitopo_remove(eng._h, None, 0, None) == 0 and eng.remove(np.zeros(0, np.uint64)) == 0
    assert eng.size() == 2498 and (eng.stat("remove_calls"), eng.stat("remove_rows")) == (1, 2)
    _same(eng.query_many(queries, 10), want)
    eng.save_index(tmp_path / "2.index")
    assert open(tmp_path / "1.index", "rb").read() == open(tmp_path / "2.index", "rb").read()
    eng.close()


def test_cpp_engine_remove_rows():
    """gpu_antitopo_engine<float>::remove_rows against a twin on the host (expann_amd/host/expann_graph_remove_check.cpp)"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "expann_amd", "host", "expann_graph_remove_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().splitlines()[-1].startswith("ok"), out.stdout


def recall_pair(seed, oracle_mod=None):
    """(repaired, fresh) recall@10 of 48 queries at ef_search 40 after 30 % of 3 000 rows were removed, against the
    oracle's brute force over the survivors"""
    import oracle_ctypes as oc
    base, q = _gauss(1000 + seed, 3000), _gauss(2000 + seed, 48)
    gone = np.random.RandomState(3000 + seed).choice(3000, 900, replace=False)
    keep = np.ones(3000, bool)
    keep[gone] = False
    truth, _ = oc.brute_force(base[keep], q, 10)
    out = []
    eng = _engine(base)
    assert eng.remove(gone) == 900
    for e in (eng, _engine(base[keep])):
        e.set_ef_search(40)
        ids, _ = e.query_many(q, 10)
        out.append(float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / 10.0 for i in range(48)])))
        e.close()
    return tuple(out)


def test_recall_guard_at_30_percent_removed():
    repaired, fresh = recall_pair(0)
    print(f"recall@10 repaired {repaired:.4f} fresh {fresh:.4f}")
    assert repaired >= fresh - RECALL_MARGIN
