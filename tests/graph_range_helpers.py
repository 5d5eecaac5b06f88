"""Yardstick of the graph engine's range search: a Python restatement of THE RANGE WALK RULE (include/expann_hip.h,
expann_graph_range_search) on the queues, the descent and the graph of tests/graph_filter_helpers.py.

  * distances are the rows of `dist_f32_matrix` (the oracle's bits), compared as the float32 values they are;
  * `range_walk_one` is the rule word for word; with predrop=True it also drops, before the queue update, what the
    kernel's pre-drop drops -- tests/test_graph_range_abi.py shows that the two forms give the same walk;
  * "d > r" is `not d <= r`: the comparison with the radius is inclusive and a NaN radius is in range of nothing;
  * the invariant of the rule is asserted after every queue update.

Nothing here touches a device."""
import numpy as np

import graph_filter_helpers as H

PAD = H.PAD
N_ROWS, M = 3000, 300
# (ef_search, max_results): the plain walk cut twice (R <= ef), and `nearest` growing past ef towards cap = R
EF_R = ((10, 8), (60, 16), (20, 256), (60, 1024))
# the radius of a query is its exact distance to its RANK-th neighbour: equal to a distance, so inclusive; in-range
# counts below ef, between ef and cap, and beyond cap over the pairs above
RANKS = (1, 10, 50, 200, 800)


def radii_at_rank(Df, rank):
    """[m] float32: each query's exact distance to its rank-th nearest row (rank 1 = the nearest)"""
    return np.ascontiguousarray(np.partition(Df, rank - 1, axis=1)[:, rank - 1])


def range_walk_one(g, df, r, R, ef, predrop=False):
    """THE RANGE WALK RULE for one query.  df[n]: its fp32 distances to every row; r: the radius.
    (ids list, dists list, count, distcomps, peak candidates size, peak nearest size)"""
    r = float(np.float32(r))
    cap = max(ef, R)
    entry, dc = H._descend(g, df)
    visited = np.zeros(g.n, bool)
    visited[entry] = True
    cand, near = H.Heap(False), H.Heap(True)
    d_entry = float(df[entry])
    dc += 1
    count = 1 if d_entry <= r else 0
    cand.push(d_entry, entry)
    near.push(d_entry, entry)
    peak_c = peak_n = 1
    adj0 = g.adj[0]
    while len(cand):
        cd, cur = cand.d[0], cand.id[0]
        if len(near) >= ef and cd > near.d[0] and (not cd <= r or len(near) >= cap):
            break
        cand.pop()
        nbs = adj0[cur]
        fresh = nbs[~visited[nbs]]  # adjacency order
        visited[fresh] = True
        dc += len(fresh)
        dns = df[fresh]
        within = dns <= np.float32(r)
        count += int(within.sum())  # counted before anything is dropped
        if predrop and len(near) >= ef:
            keep = dns < np.float32(near.d[0])
            if len(near) < cap:
                keep |= within
            fresh, dns = fresh[keep], dns[keep]
        for nb, dn in zip(fresh.tolist(), dns.tolist()):
            if len(near) < ef or dn < near.d[0] or (dn <= r and len(near) < cap):
                cand.push(dn, nb)
                near.push(dn, nb)
                peak_c, peak_n = max(peak_c, len(cand)), max(peak_n, len(near))
                if len(near) > ef and (not near.d[0] <= r or len(near) > cap):
                    near.pop()
            # the top is the largest entry: it is in range iff every entry is
            assert len(near) <= ef or (near.d[0] <= r and len(near) <= cap)
    out_d, out_id = [], []
    while len(near):
        out_d.append(near.d[0])
        out_id.append(near.id[0])
        near.pop()
    out_d.reverse()
    out_id.reverse()
    n_in = 0
    while n_in < len(out_d) and out_d[n_in] <= r:
        n_in += 1
    n_out = min(n_in, R)
    return out_id[:n_out], out_d[:n_out], count, dc, peak_c, peak_n


def range_walk(g, Df, radii, R, ef, predrop=False, rows=None):
    """queries `rows` (None: all): ids[m, R] uint64 padded, dists[m, R] float32 padded, counts[m] uint32,
    distcomps[m] uint32, peak candidates size [m], peak nearest size [m]"""
    rows = np.arange(Df.shape[0]) if rows is None else np.asarray(rows)
    m = rows.size
    ids = np.full((m, R), PAD, np.uint64)
    dists = np.full((m, R), np.inf, np.float32)
    counts, dc = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    peak_c, peak_n = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for j, i in enumerate(rows.tolist()):
        oi, od, counts[j], dc[j], peak_c[j], peak_n[j] = range_walk_one(g, Df[i], radii[i], R, ef, predrop)
        ids[j, :len(oi)] = oi
        dists[j, :len(od)] = od
    return ids, dists, counts, dc, peak_c, peak_n


def same(a, b):
    """two (ids, dists, counts, distcomps, ...) results: equal ids, distance bits, counts and distcomps"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and
            np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))
