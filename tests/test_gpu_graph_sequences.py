"""A graph engine held to THE GRAPH APPEND RULE's sentence over a sequence of appends: "every search
entry point answers bit for bit as a fresh engine that loads the saved index".

Two sequences on Gaussian rows, d = 64, M = 16, ef_construction = 80, from 3 000 rows (above the 2 048-row host route;
the settings of tests/test_gpu_graph_append.py): three appends of 150 to 400 rows, a third of them near copies of
queries, and one reserve.  Between the appends a row filter and row groups are set and cleared, the compression mode
goes through none and ranged, and query_many, grouped query_many and range_search run -- so that each append meets
the state an earlier use left on the device: a bitmap and a label array sized for the shorter graph, the ranged
walk's int8 copy and its parameters, visited sets, a filter or groups still in force.
After each append the index is saved and loaded into a fresh engine, the same filter or groups go onto both, and
every entry point is compared: ids, distance bits, counts.  The plain fp32 walk is also held to oracle.Graph on the
saved file (ids, distance bits, distcomps).  Under a filter or groups every returned id is allowed, and the answers
are those of the CPU restatements (graph_filter_helpers.py, graph_groups_helpers.py) where they apply: at these sizes
the engine's automatic "filter_flat_rows" sends every filter and every group to the exact scan, an ANY query to the
walk.  The second sequence carries a third engine over binary16 rows -- the host route -- through the same steps.
The third sequence puts a remove (the current nearest row of a third of the queries) after the first append and a
compact_row_filter (5 % tombstones and the nearest row of another third) after the second, each on the state the
appends meet -- groups and the ranged mode in force, a filter in force after the reserve: the saved file after the
call is graph_remove_helpers.apply_remove of the file before, and everything above is compared again.  Measured on
an MI355X host: 1.3 s, beside 0.5 s and 0.7 s for the first two."""
import numpy as np
import pytest

import graph_filter_helpers as H
import graph_groups_helpers as G
import graph_remove_helpers as grh

pytestmark = pytest.mark.gpu
PAD = np.uint64(2 ** 64 - 1)
D, M_EDGES, EFC, N0, N_SERIAL = 64, 16, 80, 3000, 500
MQ, K, EF, RANGE_ROWS = 48, 10, 40, 32
RESERVE = 6000   # past the three appends: none after the reserve reallocates
QGROUPS = np.asarray([5, 2, 1, G.ANY, 9, G.ABSENT], np.uint32)[np.arange(MQ) % 6]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _engine(base, rows):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M_EDGES, EFC, 1, 0, False, dim=D, rows=rows)
    eng.store_many_vectors_batched(base, False, N_SERIAL)
    eng.build()
    eng.set_ef_search(EF)
    return eng


def _load(path, rows):
    from expann_amd import AntitopoEngine
    eng = AntitopoEngine(M_EDGES, EFC, 1, 0, False, dim=D, rows=rows)
    eng.load_index(path)
    eng.set_ef_search(EF)
    return eng


def _same(a, b, what):
    assert len(a) == len(b)
    assert np.array_equal(a[0], b[0]), "%s: ids differ in rows %s" % (what, np.flatnonzero((a[0] != b[0]).any(axis=1))[:8])
    assert np.array_equal(_bits(a[1]), _bits(b[1])), "%s: distance bits differ" % what
    if len(a) > 2:
        assert np.array_equal(a[2], b[2]), "%s: counts differ" % what


class Truth:
    """what the rows say, from the oracle: every (query, row) distance, and the restatements over a saved index"""

    def __init__(self, oracle, rows, q, path):
        self.oracle, self.rows, self.q = oracle, rows, q
        self.Df = H.dist_f32_matrix(oracle, rows, q)
        self.graph = H.IndexGraph(str(path))
        self._db = {0: self.Df}

    def Db(self, mode):
        if mode not in self._db:
            self._db[mode] = H.bottom_matrix(self.oracle, self.rows, self.q, mode, self.Df)
        return self._db[mode]

    def filtered(self, allow, k):
        """the exact scan of the allowed rows: the min(k, allowed) smallest (distance, id) per query"""
        ids = np.full((MQ, k), PAD, np.uint64)
        dists = np.full((MQ, k), np.inf, np.float32)
        for i in range(MQ):
            oi, od, _ = G.scan_one(self.Df[i], allow.astype(np.uint32), 1, k)
            ids[i, :len(oi)], dists[i, :len(od)] = oi, od
        return ids, dists

    def grouped(self, labels, k, mode):
        out = G.Restatement(self.graph, self.Df, self.Db).expected(labels, QGROUPS, k, EF, mode, 0)
        return out[0], out[1], out[3]


class Pair:
    """the engine under test and, once an index has been saved, the fresh engine that loaded it: every read goes to
    both and is compared"""

    def __init__(self, oracle, base, q, rows, tmp, name):
        self.oracle, self.q, self.kind, self.tmp, self.name = oracle, q, rows, tmp, name
        self.rows = base
        self.eng = _engine(base, rows)
        self.fresh, self.truth, self.saves = None, None, 0
        self.reload()

    def reload(self):
        if self.fresh is not None:
            self.fresh.close()
        self.saves += 1
        self.path = self.tmp / ("%s_%d.index" % (self.name, self.saves))
        self.eng.save_index(self.path)
        self.fresh = _load(self.path, self.kind)
        self.truth = Truth(self.oracle, self.rows, self.q, self.path)
        self.allow = self.labels = None
        self.mode = "none"

    def engines(self):
        return (self.eng, self.fresh)

    def each(self, call):
        for e in self.engines():
            call(e)

    def set_filter(self, allow):
        self.each(lambda e: e.set_row_filter(allow))
        self.allow = allow
        if allow is not None:
            assert self.eng.stat("filter_active") == 1 and self.eng.stat("filter_rows") == int(allow.sum())

    def set_groups(self, labels):
        self.each(lambda e: e.set_row_groups(labels))
        self.labels = labels
        assert self.eng.stat("groups_active") == (labels is not None)

    def set_mode(self, mode):
        self.each(lambda e: e.set_compression(mode))
        self.mode = mode

    def query(self, k=K, what=""):
        a, b = (e.query_many(self.q, k) for e in self.engines())
        _same(a, b, "%s query_many(k=%d) %s against the loaded index" % (self.name, k, what))
        if self.allow is not None:
            real = a[0] != PAD
            assert self.allow[a[0][real].astype(np.int64)].all(), "a returned row is not allowed"
            assert (real.sum(axis=1) == np.minimum(k, int(self.allow.sum()))).all()
            _same(a, self.truth.filtered(self.allow, k), "%s filtered query_many %s against the exact scan" % (self.name, what))
        return a

    def grouped(self, k=K, what=""):
        a, b = (e.query_many(self.q, k, groups=QGROUPS) for e in self.engines())
        _same(a, b, "%s grouped query_many %s against the loaded index" % (self.name, what))
        real = a[0] != PAD
        lab = self.labels[np.where(real, a[0], 0).astype(np.int64)]
        assert ((lab == QGROUPS[:, None]) | (QGROUPS[:, None] == G.ANY) | ~real).all(), "a returned row is outside its query's group"
        mode = {"none": 0, "ranged": 2}[self.mode]
        ids, dists, classes = self.truth.grouped(self.labels, k, mode)
        assert {G.SCAN, G.WALK, G.PAD} == set(classes)
        _same(a, (ids, dists), "%s grouped query_many %s against the restatement" % (self.name, what))

    def range(self, what=""):
        radii = np.sort(self.truth.Df, axis=1)[:, [0, 4, 19, 60][self.saves % 4]].copy()
        radii[::5] = np.float32(-1.0)                        # in range of nothing
        a, b = (e.range_search(self.q, radii, RANGE_ROWS) for e in self.engines())
        _same(a, b, "%s range_search %s against the loaded index" % (self.name, what))
        real = a[0] != PAD
        got = np.take_along_axis(self.truth.Df, np.where(real, a[0], 0).astype(np.int64), axis=1)
        assert np.array_equal(_bits(got)[real], _bits(a[1])[real]) and (a[1][real] <= np.broadcast_to(radii[:, None], real.shape)[real]).all()
        assert (a[2][::5] == 0).all() and a[2].max() > 0

    def oracle_walk(self):
        """the plain fp32 walk against oracle.Graph on the saved file: ids, distance bits, distcomps"""
        og = self.oracle.Graph(str(self.path))
        for ef in (10, EF):
            oids, od, odc = og.query_k(self.q, K, ef, False)
            for e in self.engines():
                e.set_ef_search(ef)
                before = int(e.param_list()["num_distcomps"])
                _same(e.query_many(self.q, K), (oids, od), "%s query_many(ef=%d) against the oracle's walk" % (self.name, ef))
                assert int(e.param_list()["num_distcomps"]) - before == int(odc.sum()), "distcomps differ from the oracle's"

    def append(self, new):
        n0 = self.eng.size()
        assert self.eng.append(new) == len(new) and self.eng.size() == n0 + len(new)
        assert (self.eng.stat("filter_active"), self.eng.stat("groups_active"), self.eng.stat("filter_rows")) == (0, 0, n0 + len(new))
        self.eng.set_compression("none")
        self.rows = np.concatenate([self.rows, new])
        self.reload()

    def _removed(self, gone, count):
        """after a remove of the rows `gone`: the rows keep their order, the saved file is the rule's"""
        n0 = len(self.rows)
        want = grh.apply_remove(str(self.path), np.flatnonzero(gone))
        assert count == int(gone.sum()) and self.eng.size() == n0 - count
        assert (self.eng.stat("filter_active"), self.eng.stat("groups_active"), self.eng.stat("filter_rows")) == (0, 0, n0 - count)
        self.eng.set_compression("none")
        self.rows = self.rows[~gone]
        self.reload()
        grh.assert_file_is(str(self.path), want)

    def remove(self, ids):
        gone = np.zeros(len(self.rows), bool)
        gone[np.asarray(ids, np.int64)] = True
        self._removed(gone, self.eng.remove(np.asarray(ids, np.uint64)))

    def compact(self):
        """compact_row_filter under the filter in force"""
        assert self.allow is not None and self.eng.stat("filter_active") == 1
        self._removed(~self.allow, self.eng.compact_row_filter())

    def close(self):
        self.each(lambda e: e.close())


def _filter(rng, n):
    return rng.rand(n) < float(np.exp(rng.uniform(np.log(0.01), np.log(0.6))))


def _labels(rng, n):
    """label 5 on a random share of the rows, one row in group 9, 40 rows in no group, the rest in groups 2 and 1"""
    lab = np.where(rng.rand(n) < 0.7, 2, 1).astype(np.uint32)
    lab[rng.rand(n) < float(np.exp(rng.uniform(np.log(0.01), np.log(0.6))))] = 5
    pick = rng.choice(n, 41, replace=False)
    lab[pick[0]] = 9
    lab[pick[1:]] = G.ANY
    return lab


def _everything(p, rng, what):
    """every entry point, on the engine and on the fresh engine that loaded its saved index"""
    n = p.eng.size()
    p.oracle_walk()
    p.query(what=what)
    p.range(what)
    p.set_mode("ranged")
    p.query(what=what + ", ranged")
    p.set_groups(_labels(rng, n))
    p.grouped(what=what + ", ranged")
    p.set_mode("none")
    p.grouped(what=what)
    p.set_filter(_filter(rng, n))
    p.query(what=what + ", filtered")
    p.set_mode("ranged")
    p.query(what=what + ", filtered, ranged")
    p.set_mode("none")
    p.set_filter(None)
    p.set_groups(None)
    p.query(what=what + ", after the clears")


def _mutation_changed(p, before, what):
    """the sensitivity of a step: the answers of at least MQ // 4 queries changed"""
    after = p.query(what="after " + what)
    changed = int((_bits(before[1]) != _bits(after[1])).any(axis=1).sum())
    assert changed >= MQ // 4, "%s changed the answers of %d queries only" % (what, changed)


def _remove_step(p, rng, labels):
    """a remove of the current nearest row of a third of the queries, met by groups and the ranged mode in force"""
    before = p.query(what="before the remove")
    ids = np.unique(before[0][rng.choice(MQ, MQ // 3, replace=False), 0])
    p.set_groups(labels)
    p.set_mode("ranged")
    p.grouped(what="ranged, before the remove")
    p.remove(ids)
    _mutation_changed(p, before, "the remove")
    _everything(p, rng, "after the remove")


def _compact_step(p, rng):
    """a compact_row_filter: 5 % tombstones and the current nearest row of a third of the queries, met by the filter
    in force, the ranged mode and the capacity of the reserve"""
    before = p.query(what="before the compact")
    allow = rng.rand(p.eng.size()) >= 0.05
    allow[before[0][rng.choice(MQ, MQ // 3, replace=False), 0].astype(np.int64)] = False
    p.set_filter(allow)
    p.set_mode("ranged")
    p.query(what="filtered and ranged, before the compact")
    held = (p.eng.stat("capacity_rows"), p.eng.stat("graph_reallocs"))
    p.compact()
    assert held[0] == RESERVE and (p.eng.stat("capacity_rows"), p.eng.stat("graph_reallocs")) == held
    _mutation_changed(p, before, "the compact")
    _everything(p, rng, "after the compact")


@pytest.mark.parametrize("seed,with_f16,with_removes", [(1, False, False), (2, True, False), (3, False, True)],
                         ids=["f32", "f32-and-f16", "f32-with-removes"])
def test_sequence(tmp_path, oracle, seed, with_f16, with_removes):
    rng = np.random.RandomState(4100 + seed)
    base = rng.standard_normal((N0, D)).astype(np.float32)
    q = rng.standard_normal((MQ, D)).astype(np.float32)
    if with_f16:   # (rows exact in binary16, so that both engines hold the same values and one truth serves them)
        base = base.astype(np.float16).astype(np.float32)
    pairs = [Pair(oracle, base, q, "f32", tmp_path, "f32")]
    if with_f16:
        pairs.append(Pair(oracle, base, q, "f16", tmp_path, "f16"))
    sizes = [150 + rng.randint(0, 100), 300 + rng.randint(0, 100), 200 + rng.randint(0, 200)]
    try:
        for p in pairs:
            _everything(p, rng, "before the first append")
        for step, r in enumerate(sizes):
            new = rng.standard_normal((r, D)).astype(np.float32)
            near = rng.choice(MQ, MQ // 3, replace=False)    # a third of the queries get a near copy
            new[rng.choice(r, near.size, replace=False)] = q[near] + 0.01 * rng.standard_normal((near.size, D)).astype(np.float32)
            if with_f16:
                new = new.astype(np.float16).astype(np.float32)
            allow, labels = _filter(rng, pairs[0].eng.size()), _labels(rng, pairs[0].eng.size())
            for p in pairs:
                # what the append meets: step 0 a filter in force and the ranged mode, step 1 groups in force and a
                # reserve, step 2 both in force
                before = p.query(what="before append %d" % step)
                if step in (0, 2):
                    p.set_filter(allow)
                    p.query(what="filtered, before append %d" % step)
                if step in (1, 2):
                    p.set_groups(labels)
                    if step == 1:
                        p.grouped(what="before append %d" % step)
                if step == 0:
                    p.set_mode("ranged")
                    p.query(what="filtered and ranged, before append %d" % step)
                if step == 1:
                    p.eng.reserve(RESERVE)
                    p.range("after the reserve")
                held = (p.eng.stat("capacity_rows"), p.eng.stat("graph_reallocs"))
                p.append(new)
                if step >= 1 and p.kind == "f32":   # (an engine of the host route keeps no capacity)
                    assert held[0] == RESERVE and (p.eng.stat("capacity_rows"), p.eng.stat("graph_reallocs")) == held
                after = p.query(what="after append %d" % step)
                changed = int((_bits(before[1]) != _bits(after[1])).any(axis=1).sum())
                assert changed >= MQ // 4, "append %d changed the answers of %d queries only" % (step, changed)
                _everything(p, rng, "after append %d" % step)
                if with_removes and step == 0:
                    _remove_step(p, rng, _labels(rng, p.eng.size()))
                if with_removes and step == 1:
                    _compact_step(p, rng)
        f32 = pairs[0]
        assert (f32.eng.stat("append_calls"), f32.eng.stat("append_device"), f32.eng.stat("append_host")) == (3, 3, 0)
        if with_f16:
            assert (pairs[1].eng.stat("append_calls"), pairs[1].eng.stat("append_host")) == (3, 3)
        if with_removes:
            assert (f32.eng.stat("remove_calls"), f32.eng.stat("remove_device"), f32.eng.stat("remove_host")) == (2, 2, 0)
    finally:
        for p in pairs:
            p.close()
