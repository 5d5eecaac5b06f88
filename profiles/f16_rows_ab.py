"""Binary16 rows (EXPANN_DTYPE_F16) of the brute-force index: what they cost and what they save, on one MI355X.

    python profiles/f16_rows_ab.py [--parent-lib DIR] [--rocprof] [--parts 1234] > profiles/f16_rows_ab.txt

Everything resident (expann_search_device on torch tensors, the waiting form: one host wait per search), ms per
search host to host, medians of `--steps` (>= 5) timed searches after three warm ones, with [min .. max].

Part 1 (--parent-lib DIR, a directory holding the parent commit's libexpann_hip.so): the F32 path is unchanged.
  `python bench.py --gpus 1` (C2: 1 M x d128, 10 k queries, k = 10), the parent three times and this build three
  times, alternating, one process per run (EXPANN_LIB picks the library).  The acceptable difference is the
  parent's own run-to-run spread (max - min of its three values), printed next to it.
  --rocprof: one `rocprofv3 --kernel-trace --stats` run of each build over the same C2 searches (the program after
  `--`), and from its kernel statistics the summed time of the select_wave / select_topk kernels.
Part 2: F16 against F32 of the same (upcast) rows, this build, at C2's shape (there also the F32 index without its
  int8 filter, "f32 -i8f": the form an F16 index runs) and at 1 M x d768, m = 1 000, k = 100:
  ms per search, the scan kernel's device time (expann_profile), candidates per query, device bytes of the rows
  ("base_bytes") plus the fp16 filter copy.  The scan is the same code on the same bits; what differs is the
  select's re-rank over half-size rows.
Part 3: the exact scan ("scan_kernel" 1) at m = 4 and m = 64 on 1 M x d128 and 262 144 x d1024: the F16 instance
  against the F32 run-time-dim instance.  d = 128 and d = 1024 have COMPILED F32 instances, which is what an F32
  index runs; the run-time-dim F32 instance is reached at d = 144 and d = 1040 (no compiled form), so the F16
  instance is measured at all four dims and compared like for like at 144 / 1040; achieved GB/s = passes x n x d x
  element size / scan time.
Part 4: expann_add + expann_build of 1 M x d128 from host memory, F16 against F32 (upload + the prelude that makes
  the filter copy)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THIS_LIB = os.path.join(ROOT, "expann_amd", "libexpann_hip.so")


def med(ms):
    return f"{statistics.median(ms):9.3f} [{min(ms):9.3f} .. {max(ms):9.3f}]"


def rows(torch, n, d, seed=1234):
    """Gaussian rows that ARE fp16 values: the F16 index holds them, the F32 index their exact upcast"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)
    return h, g


def engine(torch, dtype, t_rows, **opts):
    from expann_amd import GpuBruteForceEngine
    eng = GpuBruteForceEngine(t_rows.shape[1], "l2", dtype)
    eng.set_base_device(t_rows.data_ptr(), t_rows.shape[0], 0)
    for name, val in opts.items():
        eng.set_option(name, val)
    eng.set_profiling(True)
    return eng


def timed(torch, eng, tq, k, steps, warm=3):
    m = tq.shape[0]
    ids = torch.empty((m, k), dtype=torch.int64, device="cuda")
    dd = torch.empty((m, k), dtype=torch.float32, device="cuda")
    out = []
    for i in range(warm + steps):
        if i == warm:
            eng.get_profile()
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.search_device(tq.data_ptr(), m, k, ids.data_ptr(), dd.data_ptr(), 0)
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out, eng.get_profile(), (ids, dd)


# ---- part 1 ------------------------------------------------------------------------------------------------------------
def worker_c2(steps):
    """the C2 searches on an F32 index, for the kernel trace (runs under either library)"""
    import torch
    h, g = rows(torch, 1_000_000, 128)
    tb = h.float()
    tq = torch.randn((10_000, 128), generator=g, device="cuda", dtype=torch.float32)
    eng = engine(torch, "f32", tb)
    ms, _, _ = timed(torch, eng, tq, 10, steps)
    eng.close()
    print(json.dumps({"ms": ms}))


def select_time_from_trace(lib, steps):
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, EXPANN_LIB=lib)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
                        os.path.abspath(__file__), "--worker-c2", "--steps", str(steps)], check=True, capture_output=True,
                       text=True, env=env)
        tot = {}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r.get("Name", "")
                for key in ("select_wave_kernel", "select_topk_kernel", "scan_gemm", "gather_logs"):
                    if key in name:
                        tot[key] = tot.get(key, 0.0) + float(r["TotalDurationNs"]) / 1e6
        return tot


def part1(parent_dir, steps, rocprof):
    libs = {"parent": os.path.join(parent_dir, "libexpann_hip.so"), "this": THIS_LIB}
    print(f"# part 1: F32 path, python bench.py --gpus 1 --steps {steps} --warmup 3 (C2), queries/s, three runs per build, alternating")
    val = {"parent": [], "this": []}
    for r in range(3):
        for name in ("parent", "this"):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                                  "3"], check=True, capture_output=True, text=True, env=dict(os.environ, EXPANN_LIB=libs[name]))
            v = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])["value"]
            val[name].append(v)
            print(f"run {r} {name:6s}: {v:12.1f} queries/s", flush=True)
    p, t = val["parent"], val["this"]
    spread = max(p) - min(p)
    delta = statistics.median(t) - statistics.median(p)
    print(f"parent: median {statistics.median(p):.1f}, run-to-run spread (max - min of three) {spread:.1f} queries/s = "
          f"{100 * spread / statistics.median(p):.2f} %; this build: median {statistics.median(t):.1f}; difference of the medians "
          f"{delta:+.1f} queries/s ({100 * delta / statistics.median(p):+.2f} %) -> "
          f"{'within' if abs(delta) <= spread or delta > 0 else 'OUTSIDE'} the parent's spread")
    if rocprof:
        print(f"# kernel trace (rocprofv3 --kernel-trace --stats), {steps + 3} C2 searches per build: summed kernel time, ms")
        for name in ("parent", "this"):
            tot = select_time_from_trace(libs[name], steps)
            print(f"{name:6s}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(tot.items())), flush=True)


# ---- part 2 ------------------------------------------------------------------------------------------------------------
def part2(steps):
    import torch
    print(f"\n# device: {torch.cuda.get_device_name(0)}")
    print("# part 2: F16 rows against F32 rows holding the same values, this build; ms per search host to host")
    print("shape                          rows | median ms [min .. max]              | scan ms  scan kernel                  "
          "cand/query | rows MB + fp16 copy MB | same ids+dists")
    for n, d, m, k in ((1_000_000, 128, 10_000, 10), (1_000_000, 768, 1_000, 100)):
        h, g = rows(torch, n, d)
        tq = torch.randn((m, d), generator=g, device="cuda", dtype=torch.float32)
        res = {}
        # (at C2's shape the F32 index takes the int8 filter of fp32 rows, which an F16 index never does: the line
        # "f32 -i8f" is the F32 index with "i8_filter" 0, the like-for-like partner of the F16 line)
        for label in ("f32", "f32 -i8f", "f16") if d == 128 else ("f32", "f16"):
            dtype = label[:3]
            tb = h.float() if dtype == "f32" else h
            eng = engine(torch, dtype, tb, **({"i8_filter": 0} if label.endswith("-i8f") else {}))
            ms, prof, out = timed(torch, eng, tq, k, steps)
            searches = steps
            base_mb = eng.get_stat("base_bytes") / 1e6
            copy_mb = n * d * 2 / 1e6
            res[dtype] = (out[0].clone(), out[1].clone())
            same = "" if dtype == "f32" else str(bool(torch.equal(res["f32"][0], res["f16"][0]) and
                                                      torch.equal(res["f32"][1].view(torch.int32), res["f16"][1].view(torch.int32))))
            print(f"{n} x d{d}, m = {m}, k = {k:<4d} {label:<8s} | {med(ms)} | {prof['scan_ms'] / searches:7.3f}  "
                  f"{prof['scan_kernel']:<28s} {prof['candidates'] / m:>10.1f} | {base_mb:8.1f} + {copy_mb:8.1f}     | {same}", flush=True)
            eng.close()
            del tb
        del h


# ---- part 3 ------------------------------------------------------------------------------------------------------------
def part3(steps):
    import torch
    print("\n# part 3: exact direct scan (\"scan_kernel\" 1), this build; scan ms = device time of the full-scan launches per search;")
    print("# GB/s = query tiles x n x d x element size / scan time (rows re-read per tile largely hit L2 / MALL: above HBM's 8 TB/s is possible)")
    print("shape                      m  rows | median ms [min .. max]              | scan ms  tiles  GB/s    | scan kernel")
    for n, dims in ((1_000_000, (128, 144)), (262_144, (1024, 1040))):
        for d in dims:
            h, g = rows(torch, n, d)
            for m in (4, 64):
                tq = torch.randn((m, d), generator=g, device="cuda", dtype=torch.float32)
                for dtype in ("f32", "f16"):
                    tb = h.float() if dtype == "f32" else h
                    eng = engine(torch, dtype, tb, scan_kernel=1)
                    ms, prof, _ = timed(torch, eng, tq, 10, steps)
                    scan = prof["scan_ms"] / max(1, prof["scan_launches"])
                    tiles = prof["scan_query_tiles"] / max(1, prof["scan_launches"])
                    gbs = tiles * n * d * (2 if dtype == "f16" else 4) / (scan * 1e-3) / 1e9 if scan > 0 else 0.0
                    print(f"{n:>9d} x d{d:<5d} {m:>6d}  {dtype} | {med(ms)} | {scan:7.3f} {tiles:6.0f} {gbs:8.1f} | {prof['scan_kernel']}",
                          flush=True)
                    eng.close()
                    del tb
            del h


# ---- part 4 ------------------------------------------------------------------------------------------------------------
def part4(steps):
    from expann_amd import GpuBruteForceEngine
    n, d = 1_000_000, 128
    base32 = np.random.default_rng(5).standard_normal((n, d), dtype=np.float32).astype(np.float16)
    print(f"\n# part 4: expann_add + expann_build of {n} x d{d} from host memory (staging copy, upload, fp16-copy prelude), ms")
    for dtype, host in (("f32", base32.astype(np.float32)), ("f16", base32)):
        add, build = [], []
        for i in range(steps + 1):
            eng = GpuBruteForceEngine(d, "l2", dtype)
            t0 = time.perf_counter()
            eng.store_many_vectors(host)
            t1 = time.perf_counter()
            eng.build()
            t2 = time.perf_counter()
            eng.close()
            if i:
                add.append((t1 - t0) * 1e3)
                build.append((t2 - t1) * 1e3)
        print(f"{dtype}: add {med(add)} | build {med(build)} | {host.nbytes / 1e6:.0f} MB uploaded", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the parent commit's build")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--parts", default="1234")
    ap.add_argument("--rocprof", action="store_true", help="part 1: also one rocprofv3 kernel trace per build")
    ap.add_argument("--worker-c2", action="store_true")
    a = ap.parse_args()
    if a.worker_c2:
        worker_c2(a.steps)
        sys.exit(0)
    assert a.steps >= 5, "medians of at least 5 repeats"
    if a.parent_lib and "1" in a.parts:  # (first: this process has not opened the device when it starts the runs)
        part1(os.path.abspath(a.parent_lib), a.steps, a.rocprof)
    if "2" in a.parts:
        part2(a.steps)
    if "3" in a.parts:
        part3(a.steps)
    if "4" in a.parts:
        part4(a.steps)
