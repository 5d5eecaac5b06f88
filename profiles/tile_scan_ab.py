"""The four tile-geometry scans (scan_tile.hpp) of this build against the parent commit's library on
one MI355X: the throughput workloads of profiles/hamming_ab.py, asym_ab.py, i4_ab.py and pq4_ab.py, and bench.py.

    python profiles/tile_scan_ab.py --parent-lib DIR [--rounds 2] [--repeats 5] > profiles/tile_scan_ab.txt

Child processes alternate (parent, this, parent, this, ...): EXPANN_LIB names DIR/libexpann_hip.so for the parent's.
A child builds each index once (1 M rows made on the device from a fixed seed), and for 10 000 queries and for 1
measures device time between two events on the search's stream around a step (the whole search: prep, thresholds,
scans, selects), one warm step and then `--repeats` steps (ten times as many for one query); k = 10.  Per workload
and side: the median and min .. max over all rounds.  A workload is "ok" when this build's median lies inside the
parent's min .. max (widened to 0.5 % either side of the parent's median where the spread is smaller), "faster"
below it and "SLOWER" above it.  bench.py (--gpus 1 --steps 60 --warmup 5)
is alternated the same way and judged by the same rule."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, MS = 1_000_000, 10, (10_000, 1)
# (form, dim, M of PQ4): the dims of the four records
WORKLOADS = ([("hamming", d, 0) for d in (256, 1024)] + [("asym", d, 0) for d in (256, 1024, 1536, 3072)] +
             [("i4", d, 0) for d in (128, 768, 3072)] + [("pq4", d, M) for d, M in ((128, 32), (768, 128), (1024, 256))])


def child(repeats):
    import numpy as np
    import torch
    from expann_amd import GpuBruteForceEngine
    st = torch.cuda.Stream()
    gen = torch.Generator(device="cuda")
    out = {}
    for form, dim, M in WORKLOADS:
        gen.manual_seed(1000 * dim + M)
        row_bytes = {"hamming": dim // 8, "asym": dim // 8, "i4": dim // 2, "pq4": M // 2}[form]
        rows = torch.randint(0, 256, (N, row_bytes), dtype=torch.uint8, device="cuda", generator=gen)
        if form == "pq4":
            cb = np.random.default_rng(dim).standard_normal((M, 16, dim // M)).astype(np.float32)
            eng = GpuBruteForceEngine(dim, "l2", "pq4", codebooks=cb)
        elif form == "i4":
            eng = GpuBruteForceEngine(dim, "ip", "i4")
        else:
            eng = GpuBruteForceEngine(dim, "hamming", "b1")
        eng.set_base_device(rows.data_ptr(), N, 0)
        if form == "hamming":
            eng.set_option("scan_kernel", 2)
        for m in MS:
            if form == "hamming":
                q = torch.randint(0, 256, (m, dim // 8), dtype=torch.uint8, device="cuda", generator=gen)
            elif form == "pq4":
                q = torch.randn((m, dim), dtype=torch.float32, device="cuda", generator=gen)
            else:
                q = torch.randint(-128, 128, (m, dim), dtype=torch.int8, device="cuda", generator=gen)
            ids = torch.empty(m, K, dtype=torch.int64, device="cuda")
            dd = torch.empty(m, K, dtype=torch.float32, device="cuda")
            call = eng.search_asym_device if form == "asym" else eng.search_device
            torch.cuda.synchronize()
            ms = []
            for r in range((repeats if m > 1 else 10 * repeats) + 1):  # (a one-query step is a fraction of a millisecond)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                call(q.data_ptr(), m, K, ids.data_ptr(), dd.data_ptr(), st.cuda_stream)
                e1.record(st)
                e1.synchronize()
                if r:  # (step 0 warms)
                    ms.append(e0.elapsed_time(e1))
            out[f"{form} dim {dim}" + (f" M {M}" if M else "") + f" m {m}"] = {
                "ms": ms, "kernel": eng.get_profile()["scan_kernel"], "ids": int(ids.sum().item())}
        eng.close()
        del rows
    print("RESULT " + json.dumps(out), flush=True)


def verdict(p, t):
    pm, tm = statistics.median(p), statistics.median(t)
    lo, hi = min(p), max(p)
    if (hi - lo) < 0.005 * pm:
        lo, hi = min(lo, 0.995 * pm), max(hi, 1.005 * pm)
    word = "faster" if tm < lo else ("SLOWER" if tm > hi else "ok")
    return f"{pm:9.3f} ({min(p):.3f} .. {max(p):.3f})   {tm:9.3f} ({min(t):.3f} .. {max(t):.3f})   {100 * (tm / pm - 1):+5.2f} %  {word}"


def run_child(cmd, lib):
    env = dict(os.environ)
    if lib:
        env["EXPANN_LIB"] = lib
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:])
        sys.exit(r.returncode or 1)
    return r.stdout


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.repeats)
        sys.exit(0)
    sides = (("parent", os.path.join(a.parent_lib, "libexpann_hip.so")), ("this", None))
    print(f"## python profiles/tile_scan_ab.py --parent-lib DIR --rounds {a.rounds} --repeats {a.repeats}")
    print(f"## 1 M rows, k = 10; ms per step: parent median (min .. max), this build median (min .. max), this / parent, verdict")
    got = {"parent": {}, "this": {}}
    same = True
    for _ in range(a.rounds):
        first = None
        for name, lib in sides:
            text = run_child([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(a.repeats)], lib)
            res = json.loads([x for x in text.splitlines() if x.startswith("RESULT ")][-1][7:])
            for key, v in res.items():
                got[name].setdefault(key, []).extend(v["ms"])
            ident = {k2: (v["kernel"], v["ids"]) for k2, v in res.items()}
            same = same and (first is None or first == ident)
            first = ident
    for key in got["parent"]:
        print(f"{key:32s} {verdict(got['parent'][key], got['this'][key])}", flush=True)
    print(f"profile kernel names and id sums of both sides: {'equal' if same else 'DIFFER'}")
    print(f"## bench.py --gpus 1 --steps 60 --warmup 5, {a.rounds} alternated rounds: ms_per_step")
    b = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, lib in sides:
            text = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "60", "--warmup", "5"], lib)
            line = json.loads([x for x in text.splitlines() if x.startswith("{")][-1])
            b[name].append(line["ms_per_step"])
            print(name, line["ms_per_step"], flush=True)
    print(f"{'bench.py':32s} {verdict(b['parent'], b['this'])}")
