"""Cases, seeded inputs and the recorder of tests/test_gpu_tile_scans.py: the four packed-row scans of the
512-row-tile geometry on the int8 matrix cores (scan_tile.hpp: Hamming, int8 queries on packed bits, 4-bit rows,
4-bit PQ) -- held to results recorded from the build in which each of them carried its own copy of the tile range,
the threshold load and the epilogue.

    python tests/tile_scans_helpers.py --record      (on the GPU, from the build whose results are the golden)

writes tests/golden/tile_scans.json: per case and k the profile's scan kernel, levels, candidate total and retries,
and an FNV-1a of the returned ids and of the distance bits.  The candidate total is the sum of the LAST level's list
lengths: it pins the keys the epilogue files there (a looser tie rule files more keys and the select hides it;
atomics permute the lists' order, never their contents).  The levels before it are pinned through the thresholds
they hand on and the final hashes; level 0's lists are fixed slots.  The recorder refuses a case with fewer than two levels or no candidates: it would pin nothing.
(65 536 rows give every form a ladder of several levels, so no form needed a larger index.)"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tile_scans.json")

# 65 536 rows: 128 tiles of 512, several levels of the ladder; + 37: a ragged last tile (padding rows, the
# row < n_rows test).  100 queries: one full query tile of 64 and a partial one of 36.
NS = (65_536, 65_536 + 37)
M = 100
KS = (10, 100)
N_DUP, N_DUP_SRC = 4096, 64   # "dup" cases: 4096 rows spread over the index are copies of 64 rows

HAM_DIMS = (64, 1024)                   # one k-step; the largest resident dim
ASYM_DIMS = (64, 576, 4096)             # a short chunk; one chunk plus one k-step; eight chunks
I4_DIMS = (64, 192, 1536)               # a short chunk; a chunk plus a short one; twelve chunks (L2 scores past 2^24 round)
PQ4_SHAPES = ((128, 16), (1024, 128), (576, 144))   # (dim, M): one chunk; the largest resident M; streamed tables


def cases():
    """[(id, spec)]: spec has form, metric, d, pq_m, n, dup and the expected profile name"""
    out = []

    def add(form, metric, d, name, pq_m=0, dup_at=None):
        tag = f"{form}-{metric}-d{d}" + (f"-M{pq_m}" if pq_m else "")
        for n in NS:
            out.append((f"{tag}-n{n}", dict(form=form, metric=metric, d=d, pq_m=pq_m, n=n, dup=False, name=name)))
        if dup_at == d:
            out.append((f"{tag}-n{NS[-1]}-dup", dict(form=form, metric=metric, d=d, pq_m=pq_m, n=NS[-1], dup=True, name=name)))
    for d in HAM_DIMS:
        add("ham", "hamming", d, "scan_hamming_mfma")
    for d in ASYM_DIMS:
        add("asym", "hamming", d, "scan_asym_mfma", dup_at=576)
    for metric in ("ip", "l2"):
        for d in I4_DIMS:
            add("i4", metric, d, "scan_i4_mfma", dup_at=1536 if metric == "l2" else None)
    for metric in ("l2", "ip"):
        for d, pq_m in PQ4_SHAPES:
            add("pq4", metric, d, "scan_pq4_mfma", pq_m=pq_m)
    return out


@functools.lru_cache(maxsize=2)
def inputs(form, d, pq_m, dup):
    """(rows [NS[-1], bytes per row] uint8 -- an index of n rows is the first n --, M queries, codebooks or None),
    seeded by form and shape"""
    rng = np.random.default_rng(9000 + 7 * d + pq_m + {"ham": 0, "asym": 1, "i4": 2, "pq4": 3}[form])
    n = NS[-1]
    cb = None
    if form in ("ham", "asym"):
        rows = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
        queries = (rng.integers(0, 256, (M, d // 8), dtype=np.uint8) if form == "ham"
                   else rng.integers(-128, 128, (M, d), dtype=np.int8))
    elif form == "i4":
        rows = rng.integers(0, 256, (n, d // 2), dtype=np.uint8)
        queries = rng.integers(-128, 128, (M, d), dtype=np.int8)
    else:
        rows = rng.integers(0, 256, (n, pq_m // 2), dtype=np.uint8)
        queries = rng.standard_normal((M, d), dtype=np.float32)
        cb = rng.standard_normal((pq_m, 16, d // pq_m), dtype=np.float32)
    if dup:   # equal scores at every rank: the tie rule (score, row) <= (tau, tau_row) decides which copies are filed
        at = rng.choice(n, N_DUP, replace=False)
        at = at[at >= N_DUP_SRC]
        rows[at] = rows[np.arange(len(at)) % N_DUP_SRC]
    return rows, queries, cb


def fnv1a(a):
    """64-bit FNV-1a over the bytes of an array, as 16 hex digits"""
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return f"{h:016x}"


def run(spec, ks):
    """the case's searches at every k of ks on one engine: {"k<k>": recorded fields}"""
    from expann_amd import GpuBruteForceEngine
    rows, queries, cb = inputs(spec["form"], spec["d"], spec["pq_m"], spec["dup"])
    dtype = {"ham": "b1", "asym": "b1", "i4": "i4", "pq4": "pq4"}[spec["form"]]
    eng = GpuBruteForceEngine(spec["d"], spec["metric"], dtype, codebooks=cb)
    eng.store_many_vectors(rows[:spec["n"]])
    eng.build()
    if spec["form"] == "ham":
        eng.set_option("scan_kernel", 2)   # the matrix-core form at every batch size
    eng.set_profiling(True)
    out = {}
    for k in ks:
        ids, dists = eng.query_k_batch_asym(queries, k) if spec["form"] == "asym" else eng.query_k_batch(queries, k)
        prof = eng.get_profile()
        out[f"k{k}"] = {"scan_kernel": prof["scan_kernel"], "levels": int(prof["levels"]),
                        "candidates": int(prof["candidates"]), "retries": int(prof["retries"]),
                        "ids": fnv1a(ids), "dists": fnv1a(dists.view(np.uint32))}
    eng.close()
    return out


def record(path):
    gold, bad = {}, []
    for cid, spec in cases():
        gold[cid] = got = run(spec, KS)
        print(cid, got, flush=True)
        for g in got.values():
            if g["scan_kernel"] != spec["name"] or g["levels"] < 2 or g["candidates"] <= 0:
                bad.append((cid, spec["name"], g))
    for b in bad:
        print("PINS NOTHING, or another kernel:", *b)
    if bad:
        return 1
    with open(path, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:2] == ["--record"]:
        sys.exit(record(sys.argv[2] if len(sys.argv) > 2 else GOLDEN))
    else:
        sys.exit("usage: tile_scans_helpers.py --record [out.json]")
