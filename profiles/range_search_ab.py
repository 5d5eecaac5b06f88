"""Range search of the brute-force index, measured on 1 M x d128 fp32 L2 rows, 10 k queries, on one MI355X.

    python profiles/range_search_ab.py --parent-lib /path/to/parent/libexpann_hip.so > profiles/range_search_ab.txt

Everything resident (torch tensors).  Times are ms of DEVICE time: HIP events on the search's stream around a call that
ends in a synchronise (so the host waits between the stages of a search are inside), medians of --repeats (>= 9)
timed calls after two warm ones, with [min .. max].
  (a) THE PLAIN SEARCH DID NOT MOVE: expann_search_device at k = 10 in the parent build and in this build, one process
      per run (EXPANN_LIB picks the library), --rounds rounds of parent then this build.  The bar is the parent's own
      min .. max.
  (b) RANGE AGAINST THE ONLY ALTERNATIVE: radii = each query's exact 10th / 100th / 1000th neighbour distance (from a
      prior search), a range search with max_results = 16 / 128 / 1024 against expann_search_device at k = 10 / 100 /
      1000, same build, same process.  The top-k search also with "i8_filter" = 0: at k = 10 this shape is inside the
      int8 filter's auto region, a family THE RANGE RULE keeps a range search out of, so that column is the top-k
      search on the kernels a range search may use.
  (c) THE DEFAULT cap0: "cand_capacity" swept over the three radii of (b).
  (d) THE SPLIT BETWEEN THE ONE-WAVE AND THE WORKGROUP FORM OF THE SELECT: EXPANN_RANGE_WAVE_MAX (lists up to that many
      keys go to the one-wave form; 0: none) swept, one process per value, default cap0."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D, M = 1_000_000, 128, 10_000
CASES = ((10, 16), (100, 128), (1000, 1024))  # (the neighbour whose distance is the radius, max_results)


def med(ms):
    return f"{statistics.median(ms):8.3f} [{min(ms):8.3f} .. {max(ms):8.3f}]"


def setup():
    import torch
    from expann_amd import GpuBruteForceEngine
    g = torch.Generator(device="cuda").manual_seed(1234)
    tb = torch.randn((N, D), generator=g, device="cuda", dtype=torch.float32)
    tq = torch.randn((M, D), generator=g, device="cuda", dtype=torch.float32)
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), N, 0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    return torch, eng, tb, tq, st


def timed(torch, st, fn, repeats, warm=2):
    out = []
    for i in range(warm + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        if i >= warm:
            out.append(e0.elapsed_time(e1))
    return out


def outputs(torch, k):
    return (torch.empty((M, k), dtype=torch.int64, device="cuda"), torch.empty((M, k), dtype=torch.float32, device="cuda"))


def worker_plain(repeats):
    torch, eng, tb, tq, st = setup()
    ids, dd = outputs(torch, 10)
    ms = timed(torch, st, lambda: eng.search_device(tq.data_ptr(), M, 10, ids.data_ptr(), dd.data_ptr(), st.cuda_stream), repeats)
    # (k = 1000, the alternative of (b)'s last row, in both builds as well: three searches after a warm one)
    ids3, dd3 = outputs(torch, 1000)
    ms3 = timed(torch, st, lambda: eng.search_device(tq.data_ptr(), M, 1000, ids3.data_ptr(), dd3.data_ptr(), st.cuda_stream), 3,
                warm=1)
    eng.close()
    print(json.dumps({"ms": ms, "ms_k1000": ms3}))


def radii_of(torch, eng, tq, st):
    """each query's exact 10th / 100th / 1000th neighbour distance, and the k = 1000 rows they come from"""
    ids, dd = outputs(torch, 1000)
    eng.search_device(tq.data_ptr(), M, 1000, ids.data_ptr(), dd.data_ptr(), st.cuda_stream)
    return {t: dd[:, t - 1].contiguous() for t, _ in CASES}, ids


def range_call(torch, eng, tq, st, radii, mr):
    ids, dd = outputs(torch, mr)
    cnt = torch.zeros(M, dtype=torch.int32, device="cuda")
    fn = lambda: eng.range_search_device(tq.data_ptr(), radii.data_ptr(), M, mr, ids.data_ptr(), dd.data_ptr(), cnt.data_ptr(),
                                         st.cuda_stream)
    return fn, ids, cnt


def worker_wave(repeats):
    torch, eng, tb, tq, st = setup()
    radii, _ = radii_of(torch, eng, tq, st)
    res = {}
    for t, mr in CASES:
        fn, _, _ = range_call(torch, eng, tq, st, radii[t], mr)
        res[t] = timed(torch, st, fn, repeats)
    eng.close()
    print(json.dumps(res))


def worker_range(repeats):
    torch, eng, tb, tq, st = setup()
    print(f"# device: {torch.cuda.get_device_name(0)}; {N} x d{D} fp32 rows, L2, {M} queries")
    radii, ref_ids = radii_of(torch, eng, tq, st)
    print("\n# (b) range search against expann_search_device at the k that holds the same rows; ms device time (top-k at k = 1000: 3 timed searches)")
    print("radius = t-th distance | max_results | range search ms                | top-k at k = t ms               | range / top-k | "
          "top-k, \"i8_filter\" = 0, ms       | mean count | retries | scan of stage 1")
    for t, mr in CASES:
        ids_k, dd_k = outputs(torch, t)
        topk = timed(torch, st, lambda: eng.search_device(tq.data_ptr(), M, t, ids_k.data_ptr(), dd_k.data_ptr(), st.cuda_stream),
                     repeats if t < 1000 else 3)
        eng.set_option("i8_filter", 0)
        topk_f16 = timed(torch, st, lambda: eng.search_device(tq.data_ptr(), M, t, ids_k.data_ptr(), dd_k.data_ptr(), st.cuda_stream),
                         repeats if t < 1000 else 3)
        eng.set_option("i8_filter", 1)
        fn, ids_r, cnt = range_call(torch, eng, tq, st, radii[t], mr)
        eng.set_profiling(True)
        fn()
        kern = eng.get_profile()["scan_kernel"]
        eng.set_profiling(False)
        rng = timed(torch, st, fn, repeats)
        agree = torch.equal(ids_r[:, :t], ids_k) and bool((cnt >= t).all())
        ratio = statistics.median(rng) / statistics.median(topk)
        print(f"{t:22d} | {mr:11d} | {med(rng)} | {med(topk)} | x {ratio:11.3f} | {med(topk_f16)} | {cnt.float().mean().item():10.2f} | "
              f"{eng.get_stat('range_retries'):7d} | {kern}{'' if agree else '   RESULTS DIFFER'}", flush=True)
    print("\n# (c) \"cand_capacity\" (cap0, the keys of a stage-1 list) swept; range search ms device time (retries of the last call)")
    print("cap0  | " + " | ".join(f"radius = {t}-th distance, max_results {mr}".ljust(42) for t, mr in CASES))
    for cap in (256, 512, 1024, 2048, 4096, 8192):
        eng.set_option("cand_capacity", cap)
        cells = []
        for t, mr in CASES:
            fn, _, _ = range_call(torch, eng, tq, st, radii[t], mr)
            ms = timed(torch, st, fn, repeats)
            cells.append(f"{med(ms)} ({eng.get_stat('range_retries'):5d})".ljust(42))
        print(f"{cap:5d} | " + " | ".join(cells), flush=True)
    eng.set_option("cand_capacity", 0)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent build's libexpann_hip.so")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return {"plain": worker_plain, "range": worker_range, "wave": worker_wave}[a.worker](a.repeats)
    assert a.repeats >= 9, "medians of at least 9 searches"
    me = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats)]
    base_env = dict(os.environ)
    base_env.pop("EXPANN_LIB", None)
    base_env.pop("EXPANN_RANGE_WAVE_MAX", None)
    if a.parent_lib:
        print(f"# (a) plain search, k = 10, {M} queries, ms device time, one process per run, {a.rounds} rounds of parent then this "
              f"build, {a.repeats} timed searches each after two warm ones")
        series = {"parent": [], "this": []}
        for r in range(a.rounds):
            for name in ("parent", "this"):
                env = dict(base_env)
                if name == "parent":
                    env["EXPANN_LIB"] = os.path.abspath(a.parent_lib)
                out = subprocess.run(me + ["--worker", "plain"], check=True, capture_output=True, text=True, env=env)
                res = json.loads(out.stdout.strip().splitlines()[-1])
                ms = res["ms"]
                series[name] += ms
                print(f"round {r} {name:6s}: {med(ms)}     k = 1000: {med(res['ms_k1000'])}", flush=True)
        p, t = series["parent"], series["this"]
        inside = min(p) <= statistics.median(t) <= max(p)
        print(f"parent: {med(p)}\nthis  : {med(t)}\nthis build's median is {'INSIDE' if inside else 'OUTSIDE'} the parent's "
              f"min .. max", flush=True)
    sys.stdout.flush()
    subprocess.run(me + ["--worker", "range"], check=True, env=base_env)
    print("\n# (d) EXPANN_RANGE_WAVE_MAX swept (lists up to that many keys: the one-wave select; 0: none), default cap0; range "
          "search ms device time")
    print("wave max | " + " | ".join(f"radius = {t}-th distance, max_results {mr}".ljust(34) for t, mr in CASES), flush=True)
    for w in (0, 128, 256, 512, 1024):
        env = dict(base_env)
        env["EXPANN_RANGE_WAVE_MAX"] = str(w)
        out = subprocess.run(me + ["--worker", "wave"], check=True, capture_output=True, text=True, env=env)
        res = json.loads(out.stdout.strip().splitlines()[-1])
        print(f"{w:8d} | " + " | ".join(med(res[str(t)]).ljust(34) for t, _ in CASES), flush=True)


if __name__ == "__main__":
    main()
