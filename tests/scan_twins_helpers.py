"""Cases, seeded inputs and the recorder of tests/test_gpu_scan_twins.py: the 16 x 16 MFMA scan kernels, fp16 and
int8 operands, of the three geometries that have (scan_gemm_w8.hpp, scan_gemm_kl.hpp) or could have
(scan_gemm_f16x.hpp / scan_gemm_i8w.hpp) one template for both -- held to results recorded from the build in
which every one of them was a hand-written kernel of its own.

    python tests/scan_twins_helpers.py --record      (on the GPU, from the build whose results are the golden)

writes tests/golden/scan_twins.json: per case and k the profile's scan kernel, candidate total and retries, and
an FNV-1a of the returned ids and of the distance bits.  The candidate total pins the filter's lists, not only
the top-k that survives the exact re-rank; atomics permute the lists' order, never their contents."""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_twins.json")

# 65 536 rows: the smallest index where the planner takes these kernels and the sampled pass has its 256 tiles
# twice over; + 37: a ragged last tile (padding rows, the row < n_rows test).  300 queries: one full query tile
# of 256 and a partial one of 44 (clamped query loads, the qi < m guards).
NS = (65_536, 65_536 + 37)
M = 300
KS = (10, 100)
REDO_RANKS = (2, 3, 4)   # tests/test_gpu_spec_tau.py's forced ranks, in the order the recorder tries them

# (dim, profile name) of the fp16 form over fp32 rows
F16_DIMS = [(64, "scan_gemm_f16x<64, false>"), (128, "scan_gemm_f16x<128, false>"),
            (256, "scan_gemm_f16y<256, false>"), (512, "scan_gemm_f16y<512, false>"),
            (80, "scan_gemm_f16kl"), (1040, "scan_gemm_f16kl")]
# (dim, profile name before the score's name) of the int8 form under scan_kernel = 5
I8_DIMS = [(128, "scan_gemm_i8w<128,"), (256, "scan_gemm_i8w<256,"), (768, "scan_gemm_i8x<768,"),
           (832, "scan_gemm_i8x<1024,"), (960, "scan_gemm_i8x<1024,"), (192, "scan_gemm_i8kl<"),
           (1088, "scan_gemm_i8kl<")]
I8_SCORES = [("u8", "l2", "U8L2"), ("i8", "l2", "I8L2"), ("i8", "ip", "I8IP")]


def cases():
    """[(id, spec)]: spec has dtype, metric, d, n, the options, the expected profile name and redo (bool)"""
    out = []
    for d, name in F16_DIMS:
        for metric in ("l2", "ip"):
            for n in NS:
                # (d = 128 L2: i8_filter = 0 keeps the fp16 form whatever the planner's auto region says)
                out.append((f"f16-{metric}-d{d}-n{n}", dict(dtype="f32", metric=metric, d=d, n=n, name=name,
                                                              opts={"i8_filter": 0}, redo=False)))
    for d, prefix in I8_DIMS:
        for dtype, metric, mn in I8_SCORES:
            for n in NS:
                out.append((f"{dtype}-{metric}-d{d}-n{n}", dict(dtype=dtype, metric=metric, d=d, n=n,
                                                                  name=prefix + mn + ">", opts={"scan_kernel": 5},
                                                                  redo=False)))
    for n in NS:
        out.append((f"redo-f16-l2-d128-n{n}", dict(dtype="f32", metric="l2", d=128, n=n, opts={"i8_filter": 0},
                                                    name="scan_gemm_f16x<128, false>", redo=True)))
        out.append((f"redo-i8f-l2-d128-n{n}", dict(dtype="f32", metric="l2", d=128, n=n, opts={"i8_filter": 2},
                                                    name="scan_gemm_i8w<128,F32L2>", redo=True)))
    return out


@functools.lru_cache(maxsize=2)
def inputs(dtype, d):
    """rows [NS[-1], d] (an index of n rows is the first n) and M queries, seeded by dtype and dim"""
    rng = np.random.default_rng(7000 + d + {"f32": 0, "u8": 1, "i8": 2}[dtype])
    n = NS[-1]
    if dtype == "f32":
        return rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((M, d), dtype=np.float32)
    if dtype == "u8":   # (uint8 rows take fp32 queries holding integers in [0, 255])
        return (rng.integers(0, 256, (n, d), dtype=np.uint8),
                rng.integers(0, 256, (M, d), dtype=np.uint8).astype(np.float32))
    return rng.integers(-128, 128, (n, d), dtype=np.int8), rng.integers(-128, 128, (M, d), dtype=np.int8)


def fnv1a(a):
    """64-bit FNV-1a over the bytes of an array, as 16 hex digits"""
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return f"{h:016x}"


def run(spec, ks, rank=None):
    """the case's searches at every k of ks on one engine (redo cases: spec_rank = rank): {"k<k>": recorded fields}"""
    from expann_amd import GpuBruteForceEngine
    base, queries = inputs(spec["dtype"], spec["d"])
    eng = GpuBruteForceEngine(spec["d"], spec["metric"], spec["dtype"])
    eng.store_many_vectors(base[:spec["n"]])
    eng.build()
    for name, val in spec["opts"].items():
        eng.set_option(name, val)
    if rank is not None:
        eng.set_option("spec_rank", rank)
    eng.set_profiling(True)
    out = {}
    for k in ks:
        ids, dists = eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        got = {"scan_kernel": prof["scan_kernel"], "candidates": int(prof["candidates"]),
               "retries": int(prof["retries"]), "ids": fnv1a(ids), "dists": fnv1a(dists.view(np.uint32))}
        if rank is not None:
            got["redo_queries"] = eng.get_stat("redo_queries")
        out[f"k{k}"] = got
    eng.close()
    return out


def record(path):
    gold, bad = {}, []
    for cid, spec in cases():
        if spec["redo"]:
            for rank in REDO_RANKS:   # the first forced rank whose redo pass really runs
                got = run(spec, (10,), rank)
                print(cid, "rank", rank, got, flush=True)
                if got["k10"]["redo_queries"] > 0 and got["k10"]["retries"] == 0:
                    break
            gold[cid] = dict(got, rank=rank)
        else:
            gold[cid] = got = run(spec, KS)
            print(cid, got, flush=True)
        for g in got.values():
            if g["scan_kernel"] != spec["name"] or g["retries"] != 0 or (spec["redo"] and not g["redo_queries"]):
                bad.append((cid, spec["name"], g))
    with open(path, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    for b in bad:
        print("NOT AS EXPECTED:", *b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:2] == ["--record"]:
        sys.exit(record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN))
    else:
        sys.exit("usage: scan_twins_helpers.py --record [out.json]")
