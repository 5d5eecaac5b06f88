"""The host model of the int8 filter's analysis (tests/i8f_model.py) against the oracle's reference-order scores,
and the adversarial constructions of tests/test_gpu_i8_filter_adversarial.py measured on it -- no GPU.

For every (query, row) pair of every construction  L <= S <= L + W_q + W_b  must hold (the analysis itself), and
each construction must really sit at the edge of it.  `bite` is the share of the half-width H = (W_q + W_b) / 2
that lies between a planted row's centre C = L + H and the smallest threshold that is still sound:

  (a) drop   (C - S_k) / H, S_k the query's k-th score: the row is dropped as soon as L = C - H exceeds tau >= S_k;
  (b) cut    (C - T) / H, T the k-th smallest decoy score: the second round keeps the row while L <= T;
  (c) tau    (S_k - C*) / (tau - C*), C* the centre the k-th largest class maximum stands for and tau the proven
             bound made from it: tau must still reach S_k.

A slack computed a factor two too small loses every pair whose bite exceeds 0.5.  Measured (minimum over the queries;
asserted with 0.05 of room): (a) 0.9865, (b) 0.9864, (c) 0.9724, (d) 0.9814 on both edge indexes (the clipped query
itself: -0.24, its error is one large component and not parallel to it -- stated, not asserted).  The algebra gives
(2c - s/2) / (2c + s/2) = 0.9874 for |q_i| = c = 39.5 s.  The iid control, the same statistic at its MAXIMUM over
the queries and their true neighbours: 0.1505 -- the data of the other int8-filter tests never comes near."""
import numpy as np
import pytest

import i8f_model as im

K = im.K


def _sub(Q, i):
    return {name: v[i:i + 1] for name, v in Q.items()}


def _assert_intervals(mod, Q, S, chunk=8):
    for i0 in range(0, S.shape[0], chunk):
        Qs = {name: v[i0:i0 + chunk] for name, v in Q.items()}
        pr = mod.pairs(Qs)
        Sd = S[i0:i0 + chunk].astype(np.float64)
        bad = (pr["L"] > Sd) | (Sd > pr["L"] + pr["width"])
        assert not bad.any(), np.argwhere(bad)[:4] + [i0, 0]


def _power_of_two_scale(mod):
    assert mod.s == 2.0 ** im.E, mod.s                        # max |x| = 127 * 2^e <= 5.5 rms: no clip, no trim


def _drop_bites(oracle, mod, base, q, fam, Q, thresholds=None):
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    assert np.array_equal(np.sort(ref[0], axis=1), np.sort(fam.astype(np.uint64), axis=1))   # the family IS the answer
    thr = ref[1][:, -1].astype(np.float64) if thresholds is None else thresholds
    bites = np.empty(len(q))
    for i in range(len(q)):
        pr = mod.pairs(_sub(Q, i), fam[i])
        bites[i] = ((pr["centre"][0] - thr[i]) / (0.5 * pr["width"][0])).min()
    return bites, ref


def test_drop_direction(oracle):
    base, q, fam, _ = im.build_drop()
    mod = im.I8fModel(base)
    _power_of_two_scale(mod)
    Q = mod.queries(q)
    _assert_intervals(mod, Q, im.all_scores(oracle, base, q))
    bites, _ = _drop_bites(oracle, mod, base, q, fam, Q)
    print(f"(a) drop: bite {bites.min():.4f} .. {bites.max():.4f}, lambda {mod.lam:.5f}")
    assert bites.min() > 0.9865 - 0.05, bites.min()


def test_cut_direction(oracle):
    base, q, fam, dec = im.build_drop(decoys=16)
    mod = im.I8fModel(base)
    _power_of_two_scale(mod)
    Q = mod.queries(q)
    S = im.all_scores(oracle, base, q)
    _assert_intervals(mod, Q, S)
    T = np.empty(len(q))
    for i in range(len(q)):
        im.assert_cut_orderings(mod, _sub(Q, i), S[i], fam[i], dec[i])
        T[i] = np.sort(S[i, dec[i]].astype(np.float64))[K - 1]
    bites, _ = _drop_bites(oracle, mod, base, q, fam, Q, thresholds=T)
    print(f"(b) cut: bite {bites.min():.4f} .. {bites.max():.4f}")
    assert bites.min() > 0.9864 - 0.05, bites.min()


def test_proven_tau_of_the_int8_sampled_pass(oracle):
    base, q, near, mid = im.build_sample()
    mod = im.I8fModel(base)
    _power_of_two_scale(mod)
    Q = mod.queries(q)
    _assert_intervals(mod, Q, im.all_scores(oracle, base, q))
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    bites = im.sample_bites(mod, Q, near, mid, ref)
    print(f"(c) proven tau: bite {bites.min():.4f} .. {bites.max():.4f}, wb_max {mod.wb_max():.1f}, w_cap {mod.w_cap:.1f}")
    assert bites.min() > 0.9724 - 0.05, bites.min()


@pytest.mark.parametrize("kind", ["clip", "clamp"])
def test_edges_of_the_integer_range(oracle, kind):
    base, q, fam = im.build_edge(kind)
    mod = im.I8fModel(base)
    assert mod.s != 2.0 ** im.E and np.abs(base).max() > im.CLIP_RMS * mod.rms        # the clip sets the scale
    Q = mod.queries(q)
    if kind == "clip":
        assert Q["M_branch_B"][0] and not Q["M_branch_B"][1:].any()                   # M_q = 2 B |e_q| for query 0 alone
        assert np.abs(q[0]).max() > 127.0 * mod.s and np.abs(base[fam[0, 0]]).max() > 127.0 * mod.s
        assert not mod.rows["clamped"].any()
    else:
        assert np.flatnonzero(mod.rows["clamped"]).tolist() == [20000] and mod.rows["bp"][20000] == im.BP_MIN
        assert np.isinf(mod.kappa(Q, np.float32(1.0), np.array([20000]))).all()       # key -inf
    _assert_intervals(mod, Q, im.all_scores(oracle, base, q))
    bites, _ = _drop_bites(oracle, mod, base, q, fam, Q)
    print(f"(d) {kind}: bite of query 0 {bites[0]:.4f}, of the others {bites[1:].min():.4f} .. {bites[1:].max():.4f}")
    assert bites[1 if kind == "clip" else 0:].min() > 0.9814 - 0.05, bites


def test_iid_control_stays_far_from_the_edge(oracle):
    base, q = im.build_iid()
    mod = im.I8fModel(base)
    Q = mod.queries(q)
    _assert_intervals(mod, Q, im.all_scores(oracle, base, q))
    ref = oracle.brute_force(base, q, K, oracle.METRIC_L2_F32, n_threads=16)
    worst = -np.inf
    for i in range(len(q)):
        pr = mod.pairs(_sub(Q, i), ref[0][i].astype(np.int64))
        worst = max(worst, ((pr["centre"][0] - float(ref[1][i, -1])) / (0.5 * pr["width"][0])).max())
    print(f"iid control: largest bite {worst:.4f}")
    assert worst < 0.2, worst
