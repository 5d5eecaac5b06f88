"""Helpers of the brute-force row-group tests: the expected answer of a grouped search is the CPU oracle over
base[groups == X] with its ids mapped back, per distinct label of the batch (ANY: the oracle over every row)."""
import os
import re

import numpy as np

PAD = np.uint64(2 ** 64 - 1)
ANY = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def list_kernel_tq():
    """the query tile of the list kernel, read from its header"""
    text = open(os.path.join(ROOT, "expann_amd", "csrc", "scan_groups.hpp")).read()
    return int(re.search(r"constexpr int kGroupScanTQ = (\d+);", text).group(1))


def expected(oracle, base, queries, k, allow, ip=False, id_offset=0):
    """the oracle over the allowed rows only, ids mapped back (PAD stays PAD)"""
    idx = np.flatnonzero(allow)
    m = queries.shape[0]
    if idx.size == 0 or m == 0:
        return np.full((m, k), PAD, np.uint64), np.full((m, k), np.inf, np.float32)
    rids, rd = oracle.brute_force(np.ascontiguousarray(base[idx]), queries, k,
                                  oracle.METRIC_IP_F32 if ip else oracle.METRIC_L2_F32, n_threads=8)
    out = np.full(rids.shape, PAD, np.uint64)
    ok = rids != PAD
    out[ok] = idx[rids[ok].astype(np.int64)].astype(np.uint64) + np.uint64(id_offset)
    return out, rd


def expected_grouped(oracle, base, groups, queries, query_groups, k, ip=False, id_offset=0):
    """one oracle call per distinct label of the batch"""
    groups = np.asarray(groups, dtype=np.uint32)
    query_groups = np.asarray(query_groups, dtype=np.uint32)
    m = queries.shape[0]
    ids = np.full((m, k), PAD, np.uint64)
    dists = np.full((m, k), np.inf, np.float32)
    for x in np.unique(query_groups):
        sel = np.flatnonzero(query_groups == x)
        allow = np.ones(groups.size, bool) if x == ANY else groups == x
        ids[sel], dists[sel] = expected(oracle, base, np.ascontiguousarray(queries[sel]), k, allow, ip, id_offset)
    return ids, dists


def same(got, want, what=""):
    ids, dists = got
    rids, rd = want
    assert np.array_equal(ids, rids), what
    assert np.array_equal(dists.view(np.uint32), rd.view(np.uint32)), what


def label_rows(n, sizes, labels, rest_labels, seed):
    """groups[n]: labels[i] on sizes[i] rows drawn at random, the other rows spread over rest_labels"""
    rng = np.random.RandomState(seed)
    order = rng.permutation(n)
    groups = np.empty(n, np.uint32)
    at = 0
    for s, lab in zip(sizes, labels):
        groups[order[at:at + s]] = lab
        at += s
    groups[order[at:]] = np.asarray(rest_labels, np.uint32)[rng.randint(0, len(rest_labels), n - at)]
    return groups


def tier_stats(eng):
    return {t: eng.get_stat("group_%s_queries" % t) for t in ("list", "filter", "any", "pad")}
