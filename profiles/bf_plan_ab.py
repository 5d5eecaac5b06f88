"""Host overhead of the brute-force planner (csrc/bf_plan.hpp), this build against another one (the parent commit's),
on one MI355X.  The two builds have the same kernels, so only the host code around the launches can differ.

    python profiles/bf_plan_ab.py --parent-lib DIR [--rounds 3] > profiles/bf_plan_ab.txt

DIR holds the other build's libexpann_hip.so.  Per round, the other build first and then this one (so the two
alternate), each in processes of its own:
  (a) `bench.py --gpus 1 --steps 60 --warmup 5`: its ms per step;
  (b) a 65 536 x d128 fp32 index: the wall time of 1 000 expann_search_device enqueues (m = 1, k = 10, "async_search"
      1) followed by one expann_sync, and the wall time of 1 000 expann_search calls from host buffers (m = 1, latency
      mode: every call plans, launches and waits); after one such block as warm-up, the median of five blocks each.
This build's median over the rounds is then compared with the smallest and the largest of the other build's runs.
Every child process runs under a time limit of its own and the first that fails ends the run."""
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


def enqueue_child():
    """(b) in this process, with whichever library EXPANN_LIB names; prints one JSON line"""
    import torch
    from expann_amd import GpuBruteForceEngine, _lib
    L = _lib.load()
    n, d, k, calls = 65536, 128, 10, 1000
    rng = np.random.default_rng(7)
    eng = GpuBruteForceEngine(d, "l2")
    eng.store_many_vectors(rng.standard_normal((n, d), dtype=np.float32))
    eng.build()
    q = rng.standard_normal((1, d), dtype=np.float32)
    st = torch.cuda.Stream()
    tq = torch.from_numpy(q).cuda()
    ids = torch.zeros((1, k), dtype=torch.int64, device="cuda")
    dists = torch.zeros((1, k), dtype=torch.float32, device="cuda")
    h_ids = np.zeros((1, k), dtype=np.uint64)
    h_dists = np.zeros((1, k), dtype=np.float32)
    torch.cuda.synchronize()

    def enqueue_block():
        t = time.perf_counter()
        for _ in range(calls):
            _lib.check(eng._h, L.expann_search_device(eng._h, tq.data_ptr(), 1, k, ids.data_ptr(), dists.data_ptr(), st.cuda_stream))
        _lib.check(eng._h, L.expann_sync(eng._h))
        return (time.perf_counter() - t) * 1e3

    def latency_block():
        t = time.perf_counter()
        for _ in range(calls):
            _lib.check(eng._h, L.expann_search(eng._h, q.ctypes.data, 1, k, h_ids.ctypes.data, h_dists.ctypes.data))
        return (time.perf_counter() - t) * 1e3
    latency_block()
    lat = [latency_block() for _ in range(5)]
    eng.set_option("async_search", 1)
    enqueue_block()
    enq = [enqueue_block() for _ in range(5)]
    out = {"enqueue_ms": enq, "latency_ms": lat, "ids": ids.cpu().numpy().ravel().tolist(), "host_ids": h_ids.ravel().tolist()}
    eng.close()
    print(json.dumps(out))


def main(parent_dir, rounds):
    import torch
    print(f"# device: {torch.cuda.get_device_name(0)}")
    builds = (("parent", parent_dir), ("this", os.path.join(ROOT, "expann_amd")))
    step_ms, enq, lat, ids = ({name: [] for name, _ in builds} for _ in range(4))
    for r in range(rounds):
        for name, lib_dir in builds:
            env = dict(os.environ, EXPANN_LIB=os.path.join(lib_dir, "libexpann_hip.so"))
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"],
                                 check=True, capture_output=True, text=True, env=env, timeout=240)
            b = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')][-1])
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--enqueue-child"], check=True,
                                 capture_output=True, text=True, env=env, timeout=120)
            e = json.loads(out.stdout.strip().splitlines()[-1])
            step_ms[name].append(b["ms_per_step"])
            enq[name].append(round(statistics.median(e["enqueue_ms"]), 3))
            lat[name].append(round(statistics.median(e["latency_ms"]), 3))
            ids[name].append(e["ids"] + e["host_ids"])
            print(f"round {r} {name:6s}: bench {b['ms_per_step']:.4f} ms per step ({b['roofline']['kernel']}); 1000 enqueues + sync "
                  f"{[round(x, 2) for x in e['enqueue_ms']]} ms; 1000 m = 1 host calls {[round(x, 2) for x in e['latency_ms']]} ms",
                  flush=True)
    assert all(x == ids["parent"][0] for x in ids["parent"] + ids["this"]), "the two builds answer differently"
    print("# the last search of every run returned the same ids in both builds")
    for label, s in (("bench ms per step", step_ms), ("1000 enqueues + sync, ms", enq), ("1000 m = 1 host calls, ms", lat)):
        p, t = s["parent"], statistics.median(s["this"])
        print(f"{label}: parent runs {p} (min {min(p)}, max {max(p)}, median {statistics.median(p)}); this build runs "
              f"{s['this']}, median {t} -> {'within' if min(p) <= t <= max(p) else 'OUTSIDE'} the parent's min-max spread")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="directory with the libexpann_hip.so of the build to compare with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--enqueue-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.enqueue_child:
        enqueue_child()
    else:
        main(os.path.abspath(a.parent_lib), a.rounds)
