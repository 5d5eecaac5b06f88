"""Host overhead of the graph handle, this build against another one (the parent commit's), on one MI355X.  The two
builds have the same kernels, so only the host code around the launches can differ.

    python profiles/graph_handle_ab.py --parent-lib DIR [--rounds 3] > profiles/graph_handle_ab.txt

DIR holds the other build's libexpann_hip.so.  Per round, the other build first and then this one (so the two
alternate), each in processes of its own:
  (a) `bench.py --gpus 1 --steps 1 --warmup 1 --workload c4`: its queries/s and ms per step;
  (b) a 4 096 x d128 SIFT-like graph (serial builder, M = 16, ef_construction = 80): the wall time of 1 000
      expann_graph_search_device enqueues (m = 1, k = 10, ef_search = 60, mode 0) followed by one expann_graph_sync,
      after one such block as warm-up; the median of five blocks is the run's figure.
This build's median over the rounds is then compared with the smallest and the largest of the other build's runs."""
import argparse
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def enqueue_child():
    """(b) in this process, with whichever library EXPANN_LIB names; prints one JSON line"""
    import torch
    from expann_amd import _lib
    from graph_device_latency import read_index_csr, sift_like
    L = _lib.load()
    n, d, k, ef, calls = 4096, 128, 10, 60, 1000
    rng = np.random.RandomState(7)
    base = sift_like(rng, n, d)
    q = sift_like(rng, 1, d, frac=True)
    with tempfile.TemporaryDirectory() as tmp:
        idx = os.path.join(tmp, "ab.index")
        e = C.c_void_p()
        assert L.expann_antitopo_create(d, 0, 16, 80, 1, 0, 0, C.byref(e)) == 0
        assert L.expann_antitopo_store(e, base.ctypes.data, n) == 0
        assert L.expann_antitopo_save(e, idx.encode()) == 0
        L.expann_antitopo_destroy(e)
        sv, n_layers, off, nb = read_index_csr(idx)
    h = C.c_void_p()
    rc = L.expann_graph_create(d, 0, base.ctypes.data, n, n_layers, sv, off.ctypes.data, nb.ctypes.data, C.byref(h))
    assert rc == 0, L.expann_graph_last_error(None)
    st = torch.cuda.Stream()
    tq = torch.from_numpy(q).cuda()
    ids = torch.zeros((1, k), dtype=torch.int64, device="cuda")
    dists = torch.zeros((1, k), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def block():
        t = time.perf_counter()
        for _ in range(calls):
            rc = L.expann_graph_search_device(h, tq.data_ptr(), 1, k, ef, 0, ids.data_ptr(), dists.data_ptr(), None,
                                              st.cuda_stream)
            assert rc == 0, L.expann_graph_last_error(h)
        assert L.expann_graph_sync(h) == 0, L.expann_graph_last_error(h)
        return (time.perf_counter() - t) * 1e3
    block()
    ms = [block() for _ in range(5)]
    L.expann_graph_destroy(h)
    print(json.dumps({"enqueue_ms": ms, "ids": ids.cpu().numpy().ravel().tolist()}))


def main(parent_dir, rounds):
    import torch
    print(f"# device: {torch.cuda.get_device_name(0)}")
    builds = (("parent", parent_dir), ("this", os.path.join(ROOT, "expann_amd")))
    qps, step_ms, enq, ids = ({name: [] for name, _ in builds} for _ in range(4))
    for r in range(rounds):
        for name, lib_dir in builds:
            env = dict(os.environ, EXPANN_LIB=os.path.join(lib_dir, "libexpann_hip.so"),
                       LD_LIBRARY_PATH=lib_dir + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
            out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1",
                                  "--workload", "c4"], check=True, capture_output=True, text=True, env=env)
            b = json.loads(out.stdout.strip().splitlines()[-1])
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--enqueue-child"], check=True,
                                 capture_output=True, text=True, env=env)
            e = json.loads(out.stdout.strip().splitlines()[-1])
            qps[name].append(b["value"])
            step_ms[name].append(b["ms_per_step"])
            enq[name].append(statistics.median(e["enqueue_ms"]))
            ids[name].append(e["ids"])
            print(f"round {r} {name:6s}: c4 {b['value']:.1f} queries/s, {b['ms_per_step']:.3f} ms per step (ef_search "
                  f"{b['config']['ef_search']}, recall {b['config']['recall']}); 1000 enqueues + sync "
                  f"{[round(x, 3) for x in e['enqueue_ms']]} ms, median {enq[name][-1]:.3f} ms", flush=True)
    assert all(x == ids["parent"][0] for x in ids["parent"] + ids["this"]), "the two builds answer differently"
    print("# the last search of every run returned the same ids in both builds")
    for label, s, unit in (("c4 queries/s", qps, ""), ("c4 ms per step", step_ms, " ms"), ("1000 enqueues + sync", enq, " ms")):
        p, t = s["parent"], statistics.median(s["this"])
        print(f"{label}: parent runs {p} (min {min(p)}, max {max(p)}, median {statistics.median(p)}){unit}; this build runs "
              f"{s['this']}, median {t}{unit} -> {'within' if min(p) <= t <= max(p) else 'OUTSIDE'} the parent's min-max spread")


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
