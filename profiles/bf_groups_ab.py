"""Row groups of the brute-force index, measured on 1 M x d128 fp32 rows, 10 k queries, k = 10, on one MI355X.

    python profiles/bf_groups_ab.py --parent-lib /path/to/parent/libexpann_hip.so > profiles/bf_groups_ab.txt

Everything resident (torch tensors; the grouped call takes its labels from host memory, as the ABI says), ms per
search HOST TO HOST (wall clock around a call that returns drained), medians of --repeats (>= 9) timed searches after
two warm ones, with [min .. max].
  (a) the PLAIN unfiltered search in this build and in the parent build: one process per run (EXPANN_LIB picks the
      library), --rounds rounds of parent then this build.  This build's median must lie inside the parent's
      min .. max: a plain search executes nothing that changed.
  (b) THE CASE THIS IS FOR: 1 000 groups of 1 000 rows, 10 queries each, in random order.  One grouped call against
      what a caller does without groups: per tenant one expann_set_row_filter plus one search of that tenant's 10
      queries (the queries sorted by tenant beforehand and the bitmaps packed beforehand: neither is timed).  The
      loop runs under the parent's library when --parent-lib is given.  The directory's set time separately.
  (c) THE CROSSOVER THAT SETS AUTO "group_list_rows": groups of 1 024 .. 16 384 rows tiling the index, 10 and 100
      queries per group, served by the list kernel ("group_list_rows" = 16384) and by filter passes (= 1).
  (d) the list kernel's device time at (b) (the handle's HIP events around its launch) beside the bytes it must read
      -- rows x 512 B once per query tile of the group -- and the keys it writes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D, M, K = 1_000_000, 128, 10_000, 10
ANY = 0xFFFFFFFF


def med(ms):
    return f"{statistics.median(ms):9.3f} [{min(ms):9.3f} .. {max(ms):9.3f}]"


def setup(n=N, m=M, more=0):
    """rows and the M queries of (a) / (b), the same in every process; `more` further queries behind them for (c)"""
    import torch
    from expann_amd import GpuBruteForceEngine
    g = torch.Generator(device="cuda").manual_seed(1234)
    tb = torch.randn((n, D), generator=g, device="cuda", dtype=torch.float32)
    tq = torch.randn((m, D), generator=g, device="cuda", dtype=torch.float32)
    if more:
        tq = torch.cat([tq, torch.randn((more, D), generator=g, device="cuda", dtype=torch.float32)])
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), n, 0)
    return torch, eng, tb, tq


def timed(torch, fn, repeats, warm=2):
    out = []
    for i in range(warm + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out


def worker_plain(repeats):
    torch, eng, tb, tq = setup()
    ids = torch.empty((M, K), dtype=torch.int64, device="cuda")
    dd = torch.empty((M, K), dtype=torch.float32, device="cuda")
    ms = timed(torch, lambda: eng.search_device(tq.data_ptr(), M, K, ids.data_ptr(), dd.data_ptr(), 0), repeats)
    eng.close()
    print(json.dumps({"ms": ms}))


def tenant_labels(n, size, seed=23):
    """groups of `size` rows drawn at random, tiling the index; the rows left over belong to no group"""
    perm = np.random.RandomState(seed).permutation(n)
    labels = np.full(n, ANY, np.uint32)
    groups = n // size
    labels[perm[:groups * size]] = np.repeat(np.arange(groups, dtype=np.uint32), size)
    return labels, groups


def worker_loop(repeats):
    """(b), the caller's loop without groups (runs under either library): JSON with the loop's wall times"""
    from expann_amd import pack_row_filter
    torch, eng, tb, tq = setup()
    labels, groups = tenant_labels(N, 1000)
    per = M // groups
    words = [pack_row_filter(labels == g) for g in range(groups)]
    ids = torch.empty((M, K), dtype=torch.int64, device="cuda")
    dd = torch.empty((M, K), dtype=torch.float32, device="cuda")
    L, h = eng._L, eng._h

    def loop():
        for g in range(groups):  # (tenant g's queries are rows [g * per, (g + 1) * per) of tq)
            w = words[g]
            assert L.expann_set_row_filter(h, w.ctypes.data, w.size) == 0
            assert L.expann_search_device(h, tq.data_ptr() + g * per * D * 4, per, K, ids.data_ptr() + g * per * K * 8,
                                          dd.data_ptr() + g * per * K * 4, None) == 0
    ms = timed(torch, loop, repeats, warm=1)
    eng.set_row_filter(None)
    eng.close()
    print(json.dumps({"ms": ms, "ids_head": ids[:per].cpu().numpy().tolist()}))


def worker_grouped(repeats, parent_lib):
    torch, eng, tb, tq = setup(more=90_000)
    print(f"# device: {torch.cuda.get_device_name(0)}; {N} x d{D} fp32 rows, k = {K}")
    # ---- (b)
    labels, groups = tenant_labels(N, 1000)
    per = M // groups
    t0 = time.perf_counter()
    eng.set_row_groups(labels)
    set_ms = (time.perf_counter() - t0) * 1e3
    rng = np.random.RandomState(5)
    order = rng.permutation(M)
    qg_sorted = np.repeat(np.arange(groups, dtype=np.uint32), per)   # tenant of query i of the loop's (sorted) array
    qg = qg_sorted[order]                                            # the grouped call: the same queries in random order
    tq_b = tq[:M][torch.from_numpy(order).cuda()].contiguous()
    ids = torch.empty((M, K), dtype=torch.int64, device="cuda")
    dd = torch.empty((M, K), dtype=torch.float32, device="cuda")
    eng.set_profiling(True)
    call = lambda: eng.search_device(tq_b.data_ptr(), M, K, ids.data_ptr(), dd.data_ptr(), 0, groups=qg)
    call()
    eng.get_profile()
    ms = timed(torch, call, repeats)
    prof = eng.get_profile()
    kern_ms = prof["scan_ms"] / (repeats + 2)
    eng.set_profiling(False)
    ms_np = timed(torch, call, repeats)
    st = {t: eng.get_stat(f"group_{t}_queries") for t in ("list", "filter", "any", "pad")}
    print(f"\n# (b) {groups} groups of 1000 rows, {per} queries each ({M} queries in random order)")
    print(f"set_row_groups (host labels, the directory made on the host): {set_ms:.1f} ms")
    print(f"one grouped call, host to host          : {med(ms_np)} ms   (tiers {st})")
    print(f"  the same with the handle's profiling on: {med(ms)} ms")
    env = dict(os.environ)
    if parent_lib:
        env["EXPANN_LIB"] = parent_lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "loop", "--repeats", str(max(3, repeats // 3))],
                         check=True, capture_output=True, text=True, env=env)
    res = json.loads(out.stdout.strip().splitlines()[-1])
    loop_ms = res["ms"]
    # (the loop's first tenant against the grouped call's rows of that tenant: the same ids)
    mine = ids.cpu().numpy()[np.argsort(order, kind="stable")][:per]
    agree = np.array_equal(np.asarray(res["ids_head"], np.int64), mine)
    print(f"{groups} x (set_row_filter + search of {per}), host to host, {'parent' if parent_lib else 'this'} build: {med(loop_ms)} ms   "
          f"(x {statistics.median(loop_ms) / statistics.median(ms_np):.1f} of the grouped call; first tenant's ids agree: {agree})")
    # ---- (d)
    tq_n = (per + 7) // 8
    rd = groups * tq_n * 1000 * D * 4
    wr = M * 1000 * 8
    print(f"\n# (d) the list kernel at (b): {kern_ms:.3f} ms device time per search (HIP events around its launch)")
    print(f"bytes it must read: {groups} groups x {tq_n} query tiles x 1000 rows x {D * 4} B = {rd / 1e6:.1f} MB; keys written: "
          f"{wr / 1e6:.1f} MB; ({rd + wr:.3e} B) / time = {(rd + wr) / (kern_ms * 1e-3) / 1e9:.1f} GB/s "
          f"(the rows themselves are {N * D * 4 / 1e6:.0f} MB: every tile after a group's first re-reads from L2 / MALL)")
    # ---- (c)
    print("\n# (c) list kernel (\"group_list_rows\" = 16384) against filter passes (\"group_list_rows\" = 1), groups tiling the index; ms host to host")
    print("group rows | groups | queries/group | list kernel ms                    | filter passes ms                  | list / filter")
    verdict = {}
    for size in (1024, 2048, 4096, 8192, 16384):
        labels, groups = tenant_labels(N, size)
        eng.set_row_groups(labels)
        for per in (10, 100):
            m = groups * per
            qg = np.repeat(np.arange(groups, dtype=np.uint32), per)[np.random.RandomState(size + per).permutation(m)]
            ids = torch.empty((m, K), dtype=torch.int64, device="cuda")
            dd = torch.empty((m, K), dtype=torch.float32, device="cuda")
            call = lambda: eng.search_device(tq.data_ptr(), m, K, ids.data_ptr(), dd.data_ptr(), 0, groups=qg)
            res, outs = {}, {}
            for way, lrows in (("list", 16384), ("filter", 1)):
                eng.set_option("group_list_rows", lrows)
                res[way] = timed(torch, call, repeats, warm=1)
                outs[way] = (ids.clone(), dd.clone())
                assert eng.get_stat(f"group_{way}_queries") == m
            same = torch.equal(outs["list"][0], outs["filter"][0]) and torch.equal(outs["list"][1].view(torch.int32),
                                                                                   outs["filter"][1].view(torch.int32))
            ratio = statistics.median(res["list"]) / statistics.median(res["filter"])
            verdict.setdefault(size, []).append(ratio)
            print(f"{size:10d} | {groups:6d} | {per:13d} | {med(res['list'])} | {med(res['filter'])} | x {ratio:.3f}"
                  f"{'' if same else '   RESULTS DIFFER'}", flush=True)
    ok = [s for s, r in verdict.items() if max(r) <= 1.0]
    print(f"# the largest measured size at which the list kernel is not slower at either load: {max(ok) if ok else 'none'}")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent build's libexpann_hip.so")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker == "plain":
        return worker_plain(a.repeats)
    if a.worker == "loop":
        return worker_loop(a.repeats)
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    if a.worker == "grouped":
        return worker_grouped(a.repeats, parent)
    assert a.repeats >= 9, "medians of at least 9 searches"
    me = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats)]
    if parent:
        print(f"# (a) plain unfiltered search, {M} queries, ms host to host, one process per run, {a.rounds} rounds of parent then "
              f"this build, {a.repeats} timed searches each after two warm ones")
        series = {"parent": [], "this": []}
        for r in range(a.rounds):
            for name in ("parent", "this"):
                env = dict(os.environ)
                env.pop("EXPANN_LIB", None)
                if name == "parent":
                    env["EXPANN_LIB"] = parent
                out = subprocess.run(me + ["--worker", "plain"], check=True, capture_output=True, text=True, env=env)
                ms = json.loads(out.stdout.strip().splitlines()[-1])["ms"]
                series[name] += ms
                print(f"round {r} {name:6s}: {med(ms)}", flush=True)
        p, t = series["parent"], series["this"]
        inside = min(p) <= statistics.median(t) <= max(p)
        print(f"parent: {med(p)}\nthis  : {med(t)}\nthis build's median is {'INSIDE' if inside else 'OUTSIDE'} the parent's "
              f"min .. max", flush=True)
    sys.stdout.flush()
    subprocess.run(me + ["--worker", "grouped"] + (["--parent-lib", parent] if parent else []), check=True)


if __name__ == "__main__":
    main()
