"""merge_topk_kernel (csrc/select.hpp) on its own: expann_merge_topk_device / _strided_device over synthetic lists
held in torch tensors, against numpy's lexsort((ids, scores))[:k] (tests/merge_helpers.py) -- ids equal, distances
equal as uint32 bit patterns.  Both instances run: the lists of a query staged in LDS (n_lists * k * 12 <= 48 KiB)
and searched where they lie (beyond); every case that matters to that switch names the instance in its id."""
import numpy as np
import pytest
import torch

from merge_helpers import PAD_ID, lists_are_well_formed, make_lists, merge_reference, staged

pytestmark = pytest.mark.gpu


def _inst(n_lists, k):
    return "lds" if staged(n_lists, k) else "global"


def _merge(ids, d, stream=None):
    """the plain form on separate [n_lists][m][k] arrays"""
    from expann_amd import merge_topk_device
    n_lists, m, k = ids.shape
    assert lists_are_well_formed(ids, d)
    ti = torch.from_numpy(ids.view(np.int64)).cuda()
    td = torch.from_numpy(d).cuda()
    oi = torch.full((m, k), 77, dtype=torch.int64, device="cuda")
    od = torch.full((m, k), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if stream is None:
        merge_topk_device(0, ti.data_ptr(), td.data_ptr(), n_lists, m, k, oi.data_ptr(), od.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            merge_topk_device(0, ti.data_ptr(), td.data_ptr(), n_lists, m, k, oi.data_ptr(), od.data_ptr(),
                              stream.cuda_stream)
        stream.synchronize()
    return oi.cpu().numpy().view(np.uint64), od.cpu().numpy()


def _check(got, ids, d, what=""):
    ri, rd = merge_reference(ids, d)
    bad = np.flatnonzero((got[0] != ri).any(1) | (got[1].view(np.uint32) != rd.view(np.uint32)).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {ri.shape[0]} queries differ, first {bad[:5]}"


# n_lists x k x m: the corners of {1, 2, 3, 8, 64} x {1, 10, 63, 64, 65, 100, 1000} x {1, 7, 300}, and every product
# n_lists * k at the switch between the two instances (4096) and just above it
GRID = [(1, 1, 1), (1, 10, 300), (1, 65, 7), (1, 1000, 7), (2, 1, 300), (2, 63, 7), (2, 64, 1), (2, 1000, 300),
        (3, 10, 7), (3, 64, 300), (3, 65, 1), (3, 100, 7), (3, 1000, 1), (8, 1, 7), (8, 10, 1), (8, 63, 300),
        (8, 65, 7), (8, 100, 300), (8, 1000, 7), (64, 1, 300), (64, 10, 7), (64, 63, 1), (64, 100, 1),
        # the switch: 4096 entries and 4097 ... , m > 1 so that a wrong query offset shows
        (64, 64, 300), (64, 65, 300), (64, 64, 1), (64, 65, 7), (8, 512, 7), (8, 513, 7), (8, 513, 300),
        (3, 2048, 7), (3, 2048, 1), (64, 1000, 7), (1, 4096, 7), (1, 4097, 7)]


@pytest.mark.parametrize("n_lists,k,m", GRID, ids=[f"{g}x{k}-m{m}-{_inst(g, k)}" for g, k, m in GRID])
def test_grid(n_lists, k, m):
    rng = np.random.RandomState(n_lists * 100_003 + k * 31 + m)
    ids, d = make_lists(rng, n_lists, m, k)
    _check(_merge(ids, d), ids, d, "full lists")
    # the same shape with lists of every length from 0 to k
    ids, d = make_lists(rng, n_lists, m, k, n_real=rng.randint(0, k + 1, size=(n_lists, m)))
    _check(_merge(ids, d), ids, d, "ragged lists")


CROSS = [(8, 100, 7), (8, 513, 7), (64, 65, 5)]
CROSS_IDS = [f"{g}x{k}-m{m}-{_inst(g, k)}" for g, k, m in CROSS]


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_negative_scores(n_lists, k, m):
    rng = np.random.RandomState(1)
    ids, d = make_lists(rng, n_lists, m, k, scores="neg", n_real=rng.randint(k // 2, k + 1, size=(n_lists, m)))
    assert (d[ids != PAD_ID] < 0).all()
    _check(_merge(ids, d), ids, d)


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_eight_distinct_scores_tie_within_and_across_lists(n_lists, k, m):
    """the order among equal scores is the id's alone"""
    rng = np.random.RandomState(2)
    ids, d = make_lists(rng, n_lists, m, k, scores="eight")
    got = _merge(ids, d)
    _check(got, ids, d)
    same = got[1][:, 1:] == got[1][:, :-1]
    assert same.any() and (got[0][:, 1:][same] > got[0][:, :-1][same]).all()


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
@pytest.mark.parametrize("where", ["two", "all"])
def test_the_same_pair_in_several_lists(n_lists, k, m, where):
    """(a shard never repeats another's id, but the merge's order is total all the same: equal pairs come out
    side by side, once per list that held them)"""
    rng = np.random.RandomState(3)
    lists = [1, n_lists - 1] if where == "two" else list(range(n_lists))
    for scores in ("gauss", "eight"):
        ids, d = make_lists(rng, n_lists, m, k, scores=scores, dup=(min(k, 20), lists))
        _check(_merge(ids, d), ids, d, scores)


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_lists_that_are_all_padding(n_lists, k, m):
    rng = np.random.RandomState(4)
    for empty in ([0], [n_lists // 2], [n_lists - 1], [0, n_lists // 2, n_lists - 1], list(range(n_lists))):
        n_real = np.full(n_lists, k)
        n_real[empty] = 0
        ids, d = make_lists(rng, n_lists, m, k, n_real=n_real)
        got = _merge(ids, d)
        _check(got, ids, d, f"empty lists {empty}")
        if len(empty) == n_lists:                  # every list all padding: the result is padding
            assert (got[0] == PAD_ID).all() and np.isposinf(got[1]).all()


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_fewer_than_k_real_entries_in_total(n_lists, k, m):
    rng = np.random.RandomState(5)
    n_real = rng.randint(0, max(1, k // n_lists), size=(n_lists, m))
    n_real[:, 0] = 0
    n_real[0, 0] = 1                               # one query has a single entry
    ids, d = make_lists(rng, n_lists, m, k, n_real=n_real)
    got = _merge(ids, d)
    _check(got, ids, d)
    total = n_real.sum(0)
    assert (total < k).all()
    for q in range(m):
        assert (got[0][q, :total[q]] != PAD_ID).all()
        assert (got[0][q, total[q]:] == PAD_ID).all() and np.isposinf(got[1][q, total[q]:]).all()


INF = [(8, 100, 7), (8, 513, 7), (16, 260, 5)]    # (3 real entries per list and more than 3 * n_lists in k)


@pytest.mark.parametrize("n_lists,k,m", INF, ids=[f"{g}x{k}-m{m}-{_inst(g, k)}" for g, k, m in INF])
def test_real_entries_scored_inf_come_before_padding(n_lists, k, m):
    rng = np.random.RandomState(6)
    per = k // n_lists - 2                         # fewer than k in total: the +inf entries reach the output
    total = per * n_lists
    assert per >= 3 and total < k
    ids, d = make_lists(rng, n_lists, m, k, n_real=per, inf_tail=2)
    got = _merge(ids, d)
    _check(got, ids, d)
    tail = got[0][:, total - 2 * n_lists:total]
    assert (tail != PAD_ID).all() and (tail[:, 1:] > tail[:, :-1]).all()
    assert np.isposinf(got[1][:, total - 2 * n_lists:]).all() and (got[0][:, total:] == PAD_ID).all()
    assert np.isfinite(got[1][:, :total - 2 * n_lists]).all()
    # and with full lists, where they compete with finite scores
    ids, d = make_lists(rng, n_lists, m, k, inf_tail=k // 2 + 1)
    _check(_merge(ids, d), ids, d, "full")


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_ids_above_2_pow_32(n_lists, k, m):
    """ids that differ only above bit 32, and only below it, with tied scores: the comparison is 64 bits wide"""
    rng = np.random.RandomState(7)
    for base, step in ((2 ** 40, 2 ** 33), (2 ** 63, 1), (2 ** 64 - 2 - 3 * n_lists * k, 3)):
        ids, d = make_lists(rng, n_lists, m, k, scores="eight", id_base=base, id_step=step)
        assert ids.min() >= 2 ** 32
        _check(_merge(ids, d), ids, d, f"ids from {base} step {step}")


def _strided(ids, d, stride_bytes, dists_off_bytes, poison=0xA5):
    """list g at byte g * stride_bytes of ONE buffer: ids first, its distances dists_off_bytes later; everything
    between the lists is poison and must stay so.  Returns (ids, dists, buffer after, buffer before)."""
    from expann_amd import merge_topk_strided_device
    n_lists, m, k = ids.shape
    assert stride_bytes % 8 == 0 and dists_off_bytes % 4 == 0 and dists_off_bytes >= m * k * 8
    assert stride_bytes >= dists_off_bytes + m * k * 4
    host = np.full(n_lists * stride_bytes, poison, np.uint8)
    for g in range(n_lists):
        o = g * stride_bytes
        host[o:o + m * k * 8] = ids[g].reshape(-1).view(np.uint8)
        host[o + dists_off_bytes:o + dists_off_bytes + m * k * 4] = d[g].reshape(-1).view(np.uint8)
    buf = torch.from_numpy(host).cuda()
    oi = torch.full((m, k), 77, dtype=torch.int64, device="cuda")
    od = torch.full((m, k), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    assert p % 8 == 0
    merge_topk_strided_device(0, p, p + dists_off_bytes, stride_bytes // 8, stride_bytes // 4, n_lists, m, k,
                              oi.data_ptr(), od.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), buf.cpu().numpy(), host


STRIDED = [(3, 10, 7), (8, 100, 7), (8, 513, 7), (5, 33, 3), (64, 65, 5)]


@pytest.mark.parametrize("n_lists,k,m", STRIDED, ids=[f"{g}x{k}-m{m}-{_inst(g, k)}" for g, k, m in STRIDED])
def test_strided_form_on_chunks_of_ids_then_dists(n_lists, k, m):
    """one buffer of [ids | dists] chunks as the sharded searches exchange them: ids_stride = chunk_bytes / 8,
    dists_stride = chunk_bytes / 4 (5 x 33 x 3: a chunk padded to 16 bytes)"""
    from expann_amd.sharded import chunk_bytes
    rng = np.random.RandomState(8)
    ids, d = make_lists(rng, n_lists, m, k, n_real=rng.randint(0, k + 1, size=(n_lists, m)))
    cb = chunk_bytes(m, k)
    gi, gd, after, before = _strided(ids, d, cb, m * k * 8)
    _check((gi, gd), ids, d)
    assert np.array_equal(after, before)


@pytest.mark.parametrize("n_lists,k,m", STRIDED, ids=[f"{g}x{k}-m{m}-{_inst(g, k)}" for g, k, m in STRIDED])
def test_strided_form_with_gaps_between_the_lists(n_lists, k, m):
    """lists spaced wider than m * k, distances not adjacent to their ids: the gaps keep their poison, whose
    bytes read as ids or scores would win every comparison (0xA5A5... as a float is a small negative number)"""
    rng = np.random.RandomState(9)
    ids, d = make_lists(rng, n_lists, m, k, n_real=rng.randint(0, k + 1, size=(n_lists, m)))
    gap = 8 * 13
    dists_off = m * k * 8 + gap
    stride = (dists_off + m * k * 4 + gap + 7) // 8 * 8
    gi, gd, after, before = _strided(ids, d, stride, dists_off)
    _check((gi, gd), ids, d)
    assert np.array_equal(after, before), "the merge wrote into its input"


@pytest.mark.parametrize("n_lists,k,m", CROSS, ids=CROSS_IDS)
def test_on_a_stream_that_is_not_the_default(n_lists, k, m):
    rng = np.random.RandomState(10)
    ids, d = make_lists(rng, n_lists, m, k, scores="eight", n_real=rng.randint(0, k + 1, size=(n_lists, m)))
    _check(_merge(ids, d, stream=torch.cuda.Stream()), ids, d)
