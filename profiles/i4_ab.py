"""4-bit rows against an int8 index of the same values (EXPANN_DTYPE_I4, scan_i4.hpp) on one MI355X.

    python profiles/i4_ab.py [--parent-lib DIR] [--parts throughput,bench] > profiles/i4_ab.txt

  throughput  1 M rows, inner product, k = 10, at dims 128, 768 and 3072, with 10 000 queries and with 1: an I4 index
              and an "i8" index of the same unpacked values in one process on one device, alternated (I4, i8, I4, i8,
              ...): device time between two events on the search's stream around a step (a step is the whole search:
              thresholds, scans, selects); one warm step each, then `--repeats` alternated steps, the median with min ..
              max; the device bytes of both; whether both return the same ids and distance bits.  The share of the int8
              MFMA peak is 2 m n dim operations over the STEP time -- an underestimate of the kernel's own share.
  bench       --parent-lib DIR: `bench.py --gpus 1 --steps 60 --warmup 5` on DIR's libexpann_hip.so and on this
              build, alternated rounds; this build's median against the other's min..max."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I8_MFMA_PEAK = 5.0e15  # int8 operations per second (dense, 2.4 GHz), as DESIGN.md 4.8 counts them


def throughput(repeats):
    import torch
    from expann_amd import GpuBruteForceEngine, pack_i4
    print("## 1 M rows, inner product, k = 10; ms per step (median, min .. max) of alternated steps; share of the int8 "
          "MFMA peak (from the step time)")
    n, k = 1_000_000, 10
    st = torch.cuda.Stream()
    for dim in (128, 768, 3072):
        rng = np.random.default_rng(dim)
        values = rng.integers(-8, 8, (n, dim), dtype=np.int8)
        t_rows = {"i4": torch.from_numpy(pack_i4(values)).cuda(), "i8": torch.from_numpy(values).cuda()}
        del values
        engines = {}
        for kind in ("i4", "i8"):
            engines[kind] = GpuBruteForceEngine(dim, "ip", kind)
            engines[kind].set_base_device(t_rows[kind].data_ptr(), n, 0)
        for m in (10_000, 1):
            tq = torch.from_numpy(rng.integers(-128, 128, (m, dim), dtype=np.int8)).cuda()
            out = {kind: (torch.empty(m, k, dtype=torch.int64, device="cuda"), torch.empty(m, k, dtype=torch.float32, device="cuda"))
                   for kind in engines}
            torch.cuda.synchronize()

            def step(kind):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                engines[kind].search_device(tq.data_ptr(), m, k, out[kind][0].data_ptr(), out[kind][1].data_ptr(), st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                return e0.elapsed_time(e1)
            ms = {kind: [] for kind in engines}
            for r in range(repeats + 1):
                for kind in engines:
                    t = step(kind)
                    if r:  # (round 0 warms both)
                        ms[kind].append(t)
            same = torch.equal(out["i4"][0], out["i8"][0]) and torch.equal(out["i4"][1].view(torch.int32), out["i8"][1].view(torch.int32))
            for kind in engines:
                med = statistics.median(ms[kind])
                print(f"dim {dim:5d} m {m:6d} {kind}: {med:10.3f} ms ({min(ms[kind]):.3f} .. {max(ms[kind]):.3f})  "
                      f"{100 * 2.0 * m * n * dim / (med * 1e-3) / I8_MFMA_PEAK:5.1f} % of the int8 MFMA peak  "
                      f"{engines[kind].get_stat('base_bytes'):12d} bytes of rows", flush=True)
            print(f"dim {dim:5d} m {m:6d}: i4 / i8 step time {statistics.median(ms['i4']) / statistics.median(ms['i8']):.2f}; "
                  f"ids and distance bits {'equal' if same else 'DIFFER'}", flush=True)
        for e in engines.values():
            e.close()


def bench(parent_lib, rounds):
    print(f"## C2 (bench.py --gpus 1 --steps 60 --warmup 5), {rounds} alternated rounds: the JSON lines, then ms_per_step")
    vals = {"parent": [], "this": []}
    for _ in range(rounds):
        for name, lib in (("parent", os.path.join(parent_lib, "libexpann_hip.so")), ("this", None)):
            env = dict(os.environ)
            if lib:
                env["EXPANN_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"],
                               env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                print(r.stderr[-2000:])
                sys.exit(r.returncode)
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            vals[name].append(line)
            print(name, json.dumps(line), flush=True)
    key = "ms_per_step"
    p, t = [x[key] for x in vals["parent"]], [x[key] for x in vals["this"]]
    print(f"{key}: parent min {min(p)} max {max(p)}; this build median {statistics.median(t)} "
          f"-> {'inside' if min(p) <= statistics.median(t) <= max(p) else 'OUTSIDE'} the parent's spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parts", default="throughput,bench")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for part in a.parts.split(","):
        if part == "bench":
            if a.parent_lib:
                bench(a.parent_lib, a.rounds)
        else:
            throughput(a.repeats)
