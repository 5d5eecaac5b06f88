"""The sharded engine creates its shards through expann_create, so it takes every f32 dim the plain
index takes: a 3-shard in-process handle at d = 1536 returns the plain index's and the oracle's ids and
fp32 distances bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_three_shards_on_one_device_d1536(oracle):
    from expann_amd import GpuBruteForceEngine, ShardedBruteForceEngine
    rng = np.random.default_rng(1536)
    n, d, m, k = 70_000, 1536, 100, 10
    base = rng.standard_normal((n, d), dtype=np.float32)
    queries = rng.standard_normal((m, d), dtype=np.float32)
    sh = ShardedBruteForceEngine(d, "l2", "f32", devices=[0, 0, 0])
    sh.store_many_vectors(base)
    sh.build()
    ids, dists = sh.query_k_batch(queries, k)
    sh.close()
    one = GpuBruteForceEngine(d, "l2")
    one.store_many_vectors(base)
    one.build()
    pids, pd = one.query_k_batch(queries, k)
    one.close()
    rids, rd = oracle.brute_force(base, queries, k, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(ids, rids) and np.array_equal(pids, rids)
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(pd.view(np.uint32), rd.view(np.uint32))
