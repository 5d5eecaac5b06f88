"""What the brute-force planner does, observed through the public ABI alone: which scan serves a search, with
which query tile, in how many levels and after how many retries, and what a refused search answers.

    python profiles/bf_plan_record.py OUT.json     runs every case on the library in use (EXPANN_LIB names another
                                                   build) and writes inputs and observations

tests/golden/bf_plan_parent.json is this file's output on the build before the planner moved to csrc/bf_plan.hpp;
tests/test_gpu_bf_plan.py replays the cases and requires the same observations field by field.  The cases are the
smallest shapes that reach each family; every case builds its own index, so none depends on another."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OPTION_DEFAULTS = {"scan_kernel": 0, "i8_filter": 1, "spec_rank": 0, "debug": 0, "cand_capacity": 0}


def case(name, dtype="f32", metric="l2", n=4096, d=128, m=24, k=10, rows="gauss", queries="gauss", rfilter=None,
         range_rank=0, **options):
    assert set(options) <= set(OPTION_DEFAULTS), options
    return dict(name=name, dtype=dtype, metric=metric, n=n, d=d, m=m, k=k, rows=rows, queries=queries, rfilter=rfilter,
                range_rank=range_rank, options=options)


def cases():
    out = []
    # the float rows' crossovers: n 4 095 / 4 096, m 4 / 5 / 24, a dim of every fp16 geometry and one without any
    for dtype in ("f32", "f16"):
        for metric in ("l2", "ip"):
            for d in (48, 64, 128, 144, 256, 768):
                for n in (4095, 4096):
                    for m in (4, 5, 24):
                        out.append(case(f"{dtype}-{metric}-d{d}-n{n}-m{m}", dtype, metric, n, d, m))
    # every "scan_kernel" on float rows (2, and 3 / 4 where no such form exists: the three refusals)
    for sk in (1, 2, 3, 4, 6):
        out.append(case(f"f32-l2-d128-sk{sk}", scan_kernel=sk))
    out.append(case("f32-l2-d256-sk3", d=256, scan_kernel=3))
    out.append(case("f32-l2-d48-sk4", d=48, scan_kernel=4))
    out.append(case("f32-ip-d128-sk3", metric="ip", scan_kernel=3))
    out.append(case("f16-l2-d128-sk3", dtype="f16", scan_kernel=3))
    out.append(case("f32-l2-d128-debug", debug=1024))  # (the instance with the ablation switches, none of them set)
    # the int8 filter of fp32 rows wherever supported, on both sides of the speculation's 64 queries
    for m in (65, 97):
        out.append(case(f"i8f-m{m}", n=32768, m=m, i8_filter=2))
        out.append(case(f"i8f-m{m}-spec4", n=32768, m=m, i8_filter=2, spec_rank=4))
    out.append(case("i8f-n32767", n=32767, m=97, i8_filter=2))
    out.append(case("f16form-m97-spec4", n=32768, m=97, i8_filter=0, spec_rank=4))
    # 8-bit rows: the direct scan, the int8 GEMM form (d = 128 only) and the q-forms (compiled, run-time dim)
    for dtype in ("u8", "i8"):
        for d in (128, 192):
            for sk in (0, 2, 5):
                for m in (95, 96):
                    out.append(case(f"{dtype}-d{d}-sk{sk}-m{m}", dtype, "l2", 65536, d, m, rows="bytes", queries="bytes",
                                    scan_kernel=sk))
    for sk in (0, 2, 5):
        out.append(case(f"i8-ip-d128-sk{sk}", "i8", "ip", 65536, 128, 96, rows="bytes", queries="bytes", scan_kernel=sk))
    out.append(case("u8-d128-n4095-m96", "u8", "l2", 4095, 128, 96, rows="bytes", queries="bytes"))
    out.append(case("u8-d128-k257", "u8", "l2", 65536, 128, 96, 257, rows="bytes", queries="bytes"))
    # the uint8 shadow of integer-valued fp32 rows, and what keeps a search off it
    out.append(case("shadow-m96", n=65536, m=96, rows="bytes", queries="bytes"))
    out.append(case("shadow-m95", n=65536, m=95, rows="bytes", queries="bytes"))
    out.append(case("shadow-n65535", n=65535, m=96, rows="bytes", queries="bytes"))
    out.append(case("shadow-real-queries", n=65536, m=96, rows="bytes", queries="gauss"))
    # a row filter: fewer allowed rows than a candidate list holds (the list path), and every other row
    out.append(case("filter-sparse", n=32768, m=32, rfilter=33))
    out.append(case("filter-dense", n=32768, m=32, rfilter=2))
    out.append(case("filter-dense-sk3", n=32768, m=32, rfilter=2, scan_kernel=3))
    # queries outside the fp16 range: fp32 rows start again on bf16x3 (d = 64 / 128) or the direct scan, fp16 rows on the direct scan
    out.append(case("far-f32-d128", n=8192, m=32, queries="far"))
    out.append(case("far-f32-d256", n=8192, d=256, m=32, queries="far"))
    out.append(case("far-f16-d128", dtype="f16", n=8192, m=32, queries="far"))
    out.append(case("far-f32-ip-d256", metric="ip", n=8192, d=256, m=32, queries="far"))
    # more equal rows than the longest candidate list holds: the filters overflow at every capacity
    out.append(case("ties-d64", n=20000, d=64, m=32, rows="ties"))
    # a range search on each side of the crossovers (radius: the range_rank-th nearest row's score)
    for n, d, m in ((4095, 128, 24), (4096, 128, 24), (4096, 144, 4), (4096, 144, 5)):
        out.append(case(f"range-d{d}-n{n}-m{m}", n=n, d=d, m=m, k=32, range_rank=10))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


@functools.lru_cache(maxsize=4)
def _values(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, d), dtype=np.float32)
    if kind == "far":  # (one component far outside the fp16 range at any scale the rows allow)
        v = rng.standard_normal((n, d), dtype=np.float32)
        v[n // 2, d // 3] = 1.0e9
        return v
    if kind == "bytes":  # integers that every 8-bit row type holds
        return rng.integers(0, 128, (n, d)).astype(np.float32)
    if kind == "ties":
        return np.tile(rng.standard_normal((1, d), dtype=np.float32), (n, 1))
    raise ValueError(kind)


def data(c):
    """(rows, queries, allow) of a case, as float32 arrays / a boolean array or None"""
    rows = _values(c["rows"], c["n"], c["d"], 1000 + c["d"])
    queries = _values(c["queries"], c["m"], c["d"], 2000 + c["d"])
    if c["dtype"] == "f16":  # (the values an F16 index holds)
        rows = rows.astype(np.float16).astype(np.float32)
    allow = None
    if c["rfilter"]:
        allow = (np.arange(c["n"]) % c["rfilter"]) == 1
    return rows, queries, allow


def run(c):
    """One case on a fresh index: (observations, ids, dists, counts); the arrays are None where the call failed."""
    from expann_amd import GpuBruteForceEngine, _lib
    rows, queries, allow = data(c)
    np_dtype = {"f32": np.float32, "f16": np.float16, "u8": np.uint8, "i8": np.int8}[c["dtype"]]
    obs = {"rc": 0, "error": ""}
    ids = dists = counts = None
    eng = None
    try:
        eng = GpuBruteForceEngine(c["d"], c["metric"], c["dtype"])
        for name, value in c["options"].items():
            eng.set_option(name, value)
        eng.store_many_vectors(rows.astype(np_dtype))
        eng.build()
        if allow is not None:
            eng.set_row_filter(allow)
        if c["range_rank"]:
            ref = _oracle_topk(c, rows, queries, None)[1]
            radii = ref[:, c["range_rank"] - 1].copy()
            ids, dists, counts = eng.range_search(queries, radii, c["k"])
        else:
            ids, dists = eng.query_k_batch(queries, c["k"])
    except _lib.ExpannError as e:
        obs["rc"] = e.code
        obs["error"] = str(e).split(": ", 1)[1]
        ids = dists = counts = None
    if eng is not None and eng._h:
        prof = eng.get_profile()
        for f in ("scan_kernel", "query_tile", "levels", "retries"):
            obs[f] = prof[f]
        for s in ("spec_rank", "i8_sample"):
            obs[s] = eng.get_stat(s)
        if c["range_rank"]:
            for s in ("range_list_queries", "range_topk_queries"):
                obs[s] = eng.get_stat(s)
        eng.close()
    return obs, ids, dists, counts


def _oracle_topk(c, rows, queries, allow):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_ctypes as oc
    metric = {("f32", "l2"): oc.METRIC_L2_F32, ("f32", "ip"): oc.METRIC_IP_F32, ("f16", "l2"): oc.METRIC_L2_F32,
              ("f16", "ip"): oc.METRIC_IP_F32, ("u8", "l2"): oc.METRIC_L2_U8, ("i8", "l2"): oc.METRIC_L2_I8,
              ("i8", "ip"): oc.METRIC_IP_I8}[(c["dtype"], c["metric"])]
    if allow is None:
        return oc.brute_force(rows, queries, c["k"], metric, n_threads=16)
    kept = np.flatnonzero(allow)
    ids, dists = oc.brute_force(rows[kept], queries, c["k"], metric, n_threads=16)
    pad = ids == np.uint64(2 ** 64 - 1)
    ids = kept.astype(np.uint64)[np.where(pad, 0, ids).astype(np.int64)]
    ids[pad] = np.uint64(2 ** 64 - 1)
    return ids, dists


def oracle(c):
    """(ids, dists, counts) the CPU oracle gives a case; counts is None for a top-k search"""
    rows, queries, allow = data(c)
    ids, dists = _oracle_topk(c, rows, queries, allow)
    if not c["range_rank"]:
        return ids, dists, None
    radii = dists[:, c["range_rank"] - 1].copy()
    rows_ids, rows_d = _oracle_topk(dict(c, k=min(c["n"], 64)), rows, queries, None)
    counts = (rows_d <= radii[:, None]).sum(axis=1).astype(np.uint32)
    assert counts.max() < rows_d.shape[1]
    keep = np.arange(c["k"])[None, :] < counts[:, None]
    ids = np.where(keep, rows_ids[:, :c["k"]], np.uint64(2 ** 64 - 1))
    dists = np.where(keep, rows_d[:, :c["k"]], np.float32(np.inf))
    return ids, dists, counts


def main(out_path):
    recorded = []
    for c in cases():
        obs, ids, dists, counts = run(c)
        recorded.append(dict(c, observed=obs))
        exact = None
        if obs["rc"] == 0:
            rids, rd, rcounts = oracle(c)
            exact = bool(np.array_equal(ids, rids) and np.array_equal(dists.view(np.uint32), rd.view(np.uint32)) and
                         (rcounts is None or np.array_equal(counts, rcounts)))
        print(c["name"], obs, "oracle:", exact, flush=True)
    with open(out_path, "w") as f:
        json.dump(recorded, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
