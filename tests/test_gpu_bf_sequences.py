"""A brute-force handle held to a plain model over random operation sequences.

Each test is one sequence of tests/bf_sequence_model.py: about 40 operations -- appends, reserves, removes, compactions,
filters, labellings, option changes and the documented refusals, interleaved with reads -- every mutation relevant to
the queries.  After EVERY mutation the driver compares size(), a search and one more entry point with the model, whose
arithmetic is the CPU oracle: ids equal, distances and scores equal as uint32 patterns, counts and status codes equal.
No tolerance appears anywhere.  tests/test_bf_sequence_model.py shows on the CPU that these sequences are sensitive,
cover the mutation sites, and that the driver fails an engine that answers from stale state.
At the end the handle is compared with a fresh engine built from the model's rows under the same options: every entry
point once more, and "copies_digest" -- the lived-in fp16 copy IS the fresh one."""
import numpy as np
import pytest

import bf_sequence_model as bsm

pytestmark = pytest.mark.gpu
CASES = [(name, seed) for name in sorted(bsm.CONFIGS) for seed in bsm.SEEDS]
NP_ROWS = {"f32": np.float32, "f16": np.float16, "u8": np.uint8, "i8": np.int8}
I8F = "scan_gemm_i8w<128,F32L2>"
# the scan forms each config must have run (prefixes of get_profile()["scan_kernel"]): the sequences reach the copies
# behind them
KERNELS = {"A": ("scan_gemm_f16x", "scan_filter_f32"),
           "B": ("scan_gemm_f16x", "scan_filter_f32", "scan_gemm_bf16x3", I8F),
           "C": ("scan_gemm_f16x", "scan_gemm_i8w<128,U8L2>"),      # (fp32 rows on the 8-bit form: the uint8 shadow)
           "D": ("scan_gemm_f16kl",),
           "E": ("scan_gemm_f16y",),
           "F": ("scan_gemm_i8<", "scan_gemm_i8w")}


@pytest.fixture(scope="module")
def gpu():
    from expann_amd import _lib
    L = _lib.load()
    assert L.expann_device_count() >= 1, "these tests need a HIP device"
    return L


def _engine(cfg, rows, options=()):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(cfg.d, cfg.metric, cfg.dtype)
    for name, val in options:
        eng.set_option(name, val)
    eng.store_many_vectors(rows)
    eng.build()
    eng.set_profiling(True)
    return eng


class Device:
    """device buffers through torch, on a side stream: rows and ids produced there, searches enqueued there"""

    def __init__(self, cfg):
        import torch
        self.torch, self.cfg = torch, cfg
        self.st = torch.cuda.Stream()

    def append(self, eng, rows):
        torch = self.torch
        rows = np.array(rows, dtype=NP_ROWS[self.cfg.dtype], order="C")   # (a copy: the sequence's arrays are read-only)
        with torch.cuda.stream(self.st):
            t = torch.from_numpy(rows).cuda(non_blocking=True)
            try:
                eng.append_device(t.data_ptr(), rows.shape[0], stream=self.st.cuda_stream)
            finally:
                t.zero_()                       # (the rows were copied: the caller may reuse its buffer on return)
                torch.cuda.synchronize()

    def remove(self, eng, ids):
        torch = self.torch
        ids = np.array(ids, dtype=np.uint64, order="C")
        with torch.cuda.stream(self.st):
            t = torch.from_numpy(ids.view(np.int64) - 1).cuda(non_blocking=True) + 1   # produced on the side stream
            try:
                return eng.remove_device(t.data_ptr(), t.numel(), stream=self.st.cuda_stream)
            finally:
                t.zero_()
                torch.cuda.synchronize()

    def enqueue(self, eng, queries, ks):
        torch = self.torch
        m = queries.shape[0]
        tq = torch.from_numpy(np.array(queries, dtype=np.float32, order="C")).cuda()
        outs = [(torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda"))
                for k in ks]
        torch.cuda.synchronize()
        eng.set_option("async_search", 1)
        for k, (tid, td) in zip(ks, outs):
            eng.search_device(tq.data_ptr(), m, k, tid.data_ptr(), td.data_ptr(), self.st.cuda_stream)
        return tq, outs

    def collect(self, eng, pending):
        eng.sync()
        self.torch.cuda.synchronize()
        eng.set_option("async_search", 0)
        return [(tid.cpu().numpy().astype(np.uint64), td.cpu().numpy()) for tid, td in pending[1]]


def _same(got, want, what):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), what


def _against_a_fresh_engine(eng, model, queries, cfg, rng):
    """every entry point once more, against an engine built from the model's rows under the same options"""
    options = tuple(model.options.items())
    fresh = _engine(cfg, model.rows.astype(NP_ROWS[cfg.dtype]), options)
    n = model.n
    assert fresh.size() == eng.size() == n
    for m, k in ((bsm.M, 10), (7, 100), (1, 1)):
        q = np.ascontiguousarray(queries[:m])
        _same(eng.query_k_batch(q, k), fresh.query_k_batch(q, k), "search(m=%d, k=%d) against a fresh engine" % (m, k))
    j = 17
    ids = model.score_case(j)
    cutoff, _ = model.expect_score(queries[j], ids)
    _same(eng.score_ids(queries[j], ids, cutoff), fresh.score_ids(queries[j], ids, cutoff), "score_ids against a fresh engine")
    d, fd = eng.get_stat("copies_digest"), fresh.get_stat("copies_digest")
    if bsm.float_rows(cfg):
        radii = model.range_radii(queries)
        _same(eng.range_search(queries, radii, bsm.RANGE_MAX_RESULTS), fresh.range_search(queries, radii, bsm.RANGE_MAX_RESULTS),
              "range search against a fresh engine")
        labels = np.asarray([3, 7, 100], np.uint32)[rng.randint(0, 3, n)]
        labels[rng.rand(n) < 0.3] = 3
        allow = rng.rand(n) < 0.2
        for e in (eng, fresh):
            e.set_row_groups(labels)
        _same(eng.query_k_batch(queries, 10, groups=bsm.QUERY_GROUPS), fresh.query_k_batch(queries, 10, groups=bsm.QUERY_GROUPS),
              "grouped search against a fresh engine")
        for e in (eng, fresh):
            e.set_row_groups(None)
            e.set_row_filter(allow)
        _same(eng.query_k_batch(queries, 10), fresh.query_k_batch(queries, 10), "filtered search against a fresh engine")
        for e in (eng, fresh):
            e.set_row_filter(None)
        if fd == 0 and n < bsm.DIRECT_BELOW:
            # below 4 096 rows a fresh index makes no fp16 copy by itself, while the handle carries the one it has: the
            # copy to compare with is made by forcing the fp16 form ("scan_kernel" 4), as test_gpu_remove.py does
            forced = _engine(cfg, model.rows.astype(NP_ROWS[cfg.dtype]), options + (("scan_kernel", 4),))
            _same(eng.query_k_batch(queries, 10), forced.query_k_batch(queries, 10), "search against the forced fp16 form")
            fd = forced.get_stat("copies_digest")
            forced.close()
        assert fd != 0 and d == fd, "copies_digest %#x, a fresh engine's %#x" % (d, fd)
    else:
        assert d == 0 and fd == 0, (d, fd)
    fresh.close()


@pytest.mark.parametrize("name,seed", CASES, ids=["%s-%d" % c for c in CASES])
def test_sequence(gpu, oracle, name, seed):
    cfg = bsm.resolve(name, seed)
    rows, queries = bsm.initial(name, seed)
    ops = bsm.generate(name, seed)
    model = bsm.Model(oracle, cfg, rows)
    eng = _engine(cfg, rows)
    device = Device(cfg) if bsm.CONFIGS[name].async_seed == seed else None
    by_step = {}

    def after_step(i, op, drv):
        by_step[i] = eng.get_profile()["scan_kernel"]   # (the last full scan of the step; "" when it launched none)

    try:
        bsm.run(eng, model, ops, oracle, queries=queries, device=device, config=name, seed=seed, after_step=after_step)
        kernels = set(by_step.values())
        stats = {s: eng.get_stat(s) for s in ("append_extends", "append_rebuilds", "remove_compacts", "remove_rebuilds",
                                              "base_reallocs", "base_capacity_rows")}
        print("sequence %s-%d: %d rows at the end; scan kernels %s; %s" % (name, seed, model.n, sorted(kernels), stats))
        _against_a_fresh_engine(eng, model, queries, cfg, np.random.RandomState(seed))
    finally:
        eng.close()
    for prefix in KERNELS[name]:
        assert any(kn.startswith(prefix) for kn in kernels), (prefix, sorted(kernels))
    batches = [i for i, op in enumerate(ops) if op["op"] == "search" and (op["m"], op["k"]) == (bsm.M, 10)]
    if name == "B":
        # the int8 filter's set was built, forgotten by a remove and by an append, and built again each time
        assert sum(by_step[i] == I8F for i in batches) >= 3, [by_step[i] for i in batches]
    if name == "C":
        # the uint8 shadow served the batch before the fractional row came, and not the batch after it
        odd = max(i for i, op in enumerate(ops) if op["op"] == "append")
        assert "U8L2" in by_step[odd - 1] and by_step[odd + 1].startswith("scan_gemm_f16x"), (by_step[odd - 1], by_step[odd + 1])
    if bsm.float_rows(cfg):
        # the fp16 copy lived through the sequence: extended and compacted in place, dropped where the scale changed
        assert stats["append_extends"] >= 1 and stats["remove_compacts"] >= 1, stats
        assert stats["append_rebuilds"] + stats["remove_rebuilds"] >= 1, stats
