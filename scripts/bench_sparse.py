"""CSR rows (ti_predict_csr) beside the dense path on the rows they stand for.

One resident forest: 500 seeded XGBoost trees of depth 6 whose splits fall on
128 columns of a 20,000-column matrix (so the sparse image holds U <= 128
columns: regime A at 128-row tiles of float32 values).  One batch: 100,000 rows,
1 % of the entries stored, N(0,1) float32 values, every one of a row's used
columns stored with the same 1 % chance as any other.  Three host-to-host
calls are timed on it, each ending in the library's own stream synchronise:

  csr_image   ti_predict_csr, the LDS image (regime A)
  csr_search  ti_predict_csr under TI_SPARSE_SEARCH=1 (regime B)
  dense       ti_predict on the densified float32 rows (absent = NaN), 8 GB at
              the default size: --dense-rows densifies only the first so many
              rows and the line says so

Host wall clock around whole calls (the copies in and out are what a caller
pays), the three alternating round by round, each round a window of at least a
quarter of a second; a line with each call's median, minimum, maximum and
spread (max - min) / median goes to stdout and to --out.  The margins of the
three are compared bit for bit before anything is timed.

Usage: python scripts/bench_sparse.py [--rows 100000] [--dense-rows 100000]
           [--rounds 7] [--out profiles/sparse_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TI_DEV_KNOBS"] = "1"
TREES, DEPTH, USED, COLS, DENSITY = 500, 6, 128, 20000, 0.01


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=100000)
    p.add_argument("--dense-rows", type=int, default=100000)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.jsonl"))
    a = p.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_MARGIN
    from kfserving_amd.formats import xgboost_format as xf
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    trees, ti = xf.synthetic_complete_trees(TREES, DEPTH, USED, seed=17)
    rng = np.random.default_rng(17)
    pool = np.sort(rng.choice(COLS, USED, replace=False)).astype(np.uint32)
    for t in trees:
        s = t["sindex"][:(1 << DEPTH) - 1]
        s[:] = pool[s & 0x7fffffff] | (s & 0x80000000)
    dev = DeviceForest(xf.forest_from_raw_trees(trees, ti, COLS, 0, 0.0, "binary:logistic"), [0])
    n, nd = a.rows, min(a.dense_rows, a.rows)
    draws = rng.binomial(COLS, DENSITY, size=n)   # a row's repeated draws fall together
    keys = np.unique(np.repeat(np.arange(n, dtype=np.int64), draws) * COLS +
                     rng.integers(0, COLS, size=int(draws.sum())))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(keys // COLS, minlength=n))]).astype(np.int64)
    indices = (keys % COLS).astype(np.int32)
    S = sp.csr_matrix((rng.standard_normal(indptr[-1]).astype(np.float32), indices, indptr),
                      shape=(n, COLS))
    D = np.full((nd, COLS), np.nan, dtype=np.float32)
    head = S[:nd].tocoo()
    D[head.row, head.col] = head.data

    def call(k):
        if k == "dense":
            return dev.predict(D, OUT_MARGIN)
        os.environ["TI_SPARSE_SEARCH"] = "1" if k == "csr_search" else "0"
        return dev.predict(S, OUT_MARGIN, absent="nan")
    names = ("csr_image", "csr_search", "dense")
    first = {k: call(k) for k in names}
    info = dev.info()
    if not (np.array_equal(first["csr_image"], first["csr_search"]) and
            np.array_equal(first["csr_image"][:nd], first["dense"])):
        raise SystemExit("the three calls' margins differ: nothing to time")

    def window(k, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            call(k)
        return (time.perf_counter() - t0) * 1e3 / reps
    reps = {k: max(1, int(250.0 / max(window(k, 1), 1e-3))) for k in names}   # also the warm-up
    ms = {k: [] for k in names}
    for _ in range(a.rounds):
        for k in names:        # alternating: the three see the same drift
            ms[k].append(window(k, reps[k]))
    rec = {"rows": n, "dense_rows": nd, "cols": COLS, "density": DENSITY, "nnz": int(indptr[-1]),
           "trees": TREES, "depth": DEPTH, "x": "float32", "rounds": a.rounds,
           "sparse_cols": info["sparse_cols"], "layout": info["layout"],
           "bit_identical_margins": True, "clock": "host wall, whole calls"}
    for k in names:
        med = statistics.median(ms[k])
        rows_k = nd if k == "dense" else n
        rec[k] = {"reps": reps[k], "ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                  "spread": (max(ms[k]) - min(ms[k])) / med, "rows_per_s": rows_k / (med * 1e-3)}
    rec["dense_over_csr_image_per_row"] = (rec["dense"]["ms_median"] / nd) / (rec["csr_image"]["ms_median"] / n)
    rec["csr_search_over_csr_image"] = rec["csr_search"]["ms_median"] / rec["csr_image"]["ms_median"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
