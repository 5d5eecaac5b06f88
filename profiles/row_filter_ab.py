"""Row filter of the brute-force engine: what it costs, on one MI355X.

    python profiles/row_filter_ab.py [--parent-lib DIR] > profiles/row_filter_ab.txt

Shape: 1 M x d128 Gaussian rows, 10 k queries, k = 10, everything resident (expann_search_device on torch tensors,
the waiting form: one host wait per search), host-to-host ms per search.

Part 1 (--parent-lib DIR, a directory holding another build's libexpann_hip.so): the UNFILTERED search, the other
build and this one alternating, one process per run (EXPANN_LIB picks the library), `--steps` timed searches per
run after three warm ones.  The existing kernels and their launch paths are untouched, so the difference of the
medians should lie within the parent's own spread (max - min of its runs).
Part 2: this build, filtered against unfiltered: random filters of density 50 %, 5 % and 0.1 % (1 000 rows: the
list path), with the profile's kernel name, candidates per query and retries.  (The unfiltered search of this
shape takes the int8 filter of fp32 rows, which a filtered search never does: the filtered lines run the fp16 form.)
Part 3: host-to-host time of expann_set_row_filter_device at 1 M rows (bits already in device memory)."""
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


def setup():
    import torch
    from expann_amd import GpuBruteForceEngine
    g = torch.Generator(device="cuda").manual_seed(1234)
    tb = torch.randn((N, D), generator=g, device="cuda", dtype=torch.float32)
    tq = torch.randn((M, D), generator=g, device="cuda", dtype=torch.float32)
    ids = torch.empty((M, K), dtype=torch.int64, device="cuda")
    dd = torch.empty((M, K), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng = GpuBruteForceEngine(D, "l2")
    eng.set_base_device(tb.data_ptr(), N, 0)
    return torch, eng, (tb, tq, ids, dd)


def timed(torch, eng, bufs, steps, warm=3):
    _, tq, ids, dd = bufs
    out = []
    for i in range(warm + steps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.search_device(tq.data_ptr(), M, K, ids.data_ptr(), dd.data_ptr(), 0)
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out


def worker_unfiltered(steps):
    torch, eng, bufs = setup()
    print(json.dumps({"ms": timed(torch, eng, bufs, steps)}))


def part1(parent_dir, rounds, steps):
    series = {"parent": [], "this": []}
    libs = {"parent": os.path.join(parent_dir, "libexpann_hip.so"), "this": os.path.join(ROOT, "expann_amd", "libexpann_hip.so")}
    print(f"# part 1: unfiltered search, {N} x d{D}, {M} queries, k = {K}; {rounds} runs of {steps} timed searches per build, "
          "alternating, one process per run")
    for r in range(rounds):
        for name in ("parent", "this"):
            env = dict(os.environ, EXPANN_LIB=libs[name])
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps)], check=True,
                                 capture_output=True, text=True, env=env)
            ms = json.loads(out.stdout.strip().splitlines()[-1])["ms"]
            series[name] += ms
            print(f"run {r} {name:6s}: median {statistics.median(ms):.3f} ms  [{min(ms):.3f} .. {max(ms):.3f}]", flush=True)
    p, t = series["parent"], series["this"]
    spread = max(p) - min(p)
    delta = statistics.median(t) - statistics.median(p)
    print(f"parent: median {statistics.median(p):.3f} ms over {len(p)} searches, spread (max - min) {spread:.3f} ms; this build: "
          f"median {statistics.median(t):.3f} ms over {len(t)}; difference of the medians {delta:+.3f} ms -> "
          f"{'within' if abs(delta) <= spread else 'OUTSIDE'} the parent's spread")


def part23(steps):
    from expann_amd import pack_row_filter
    torch, eng, bufs = setup()
    eng.set_profiling(True)
    print(f"\n# device: {torch.cuda.get_device_name(0)}")
    print(f"# part 2: this build, {N} x d{D}, {M} queries, k = {K}, {steps} timed searches per line (ms, host to host)")
    print("filter      allowed rows | median ms [min .. max]        | scan kernel                      cand / query  retries")
    rng = np.random.RandomState(5)
    tbits = None
    for density in (None, 0.5, 0.05, 0.001):
        if density is None:
            eng.set_row_filter(None)
        else:
            allow = rng.rand(N) < density
            tbits = torch.from_numpy(pack_row_filter(allow).view(np.int32)).cuda()
            torch.cuda.synchronize()
            eng.set_row_filter_device(tbits.data_ptr(), tbits.numel(), 0)
        eng.get_profile()
        ms = timed(torch, eng, bufs, steps)
        prof = eng.get_profile()
        searches = steps + 3
        label = "none" if density is None else f"{100 * density:g} %"
        print(f"{label:<11s} {eng.get_stat('filter_rows'):>12d} | {statistics.median(ms):8.3f} [{min(ms):8.3f} .. {max(ms):8.3f}] | "
              f"{prof['scan_kernel']:<32s} {prof['candidates'] / M:>12.1f} {prof['retries'] / searches:>8.2f}", flush=True)
    print(f"\n# part 3: expann_set_row_filter_device at {N} rows ({tbits.numel() * 4} bytes of bits in device memory), host to host")
    us = []
    for _ in range(23):
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.set_row_filter_device(tbits.data_ptr(), tbits.numel(), 0)
        us.append((time.perf_counter() - t) * 1e6)
    us = us[3:]
    print(f"median {statistics.median(us):.1f} us [{min(us):.1f} .. {max(us):.1f}] over {len(us)} calls (the masked row terms "
          "are rebuilt by the next search: two passes over 4 MB)")
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the build to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        worker_unfiltered(a.steps)
        sys.exit(0)
    if a.parent_lib:  # (first: this process has not opened the device when it starts the runs)
        part1(os.path.abspath(a.parent_lib), a.rounds, a.steps)
    part23(a.steps)
