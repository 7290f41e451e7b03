"""K-Means / weighted filters: the device path against the host path it replaces, one process, one clock.

    python tools/kmeans_bench.py [--runs 5] [--out kmeans_bench.json]

Per shape (1024, 51) and (2048, 102), plain and weighted: wall time of the whole ``kmeans_queries`` call between two device
synchronisations (the call has host read-backs inside, so stream events alone would flatter it), one warm-up call, median of
``--runs``, on the same device rows.  The host path gets what it needed before: the float64 copy of the rows to the host, then
scikit-learn.  Thread counts are left as the machine sets them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vatl4pose-wacv2024_amd"))
sys.path.insert(0, ROOT)

from active_learning import query as Q  # noqa: E402
from tests.kmeans_cases import emb, weights  # noqa: E402


def timed(fn, runs):
    fn()                                                         # warm-up
    out = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
    ap.add_argument("--device-only", action="store_true", help="skip the host path (for a kernel trace of the device path)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for n, k, seed in ((1024, 51, 3), (2048, 102, 11)):
        x = torch.from_numpy(emb(n, seed=seed)).to(dev)
        cand = list(range(n))
        for weighted in (False, True):
            w = weights(n, seed) if weighted else None
            d_ms, d_res = timed(lambda: Q.kmeans_queries(x, cand, k, w), a.runs)
            row = {"n": n, "k": k, "weighted": weighted, "device_ms": round(d_ms, 3), "device_path": d_res.path, "device_iters": d_res.n_iter}
            if not a.device_only:
                h_ms, h_res = timed(lambda: Q.kmeans_queries(x.double().cpu().numpy(), cand, k, w), a.runs)
                row.update(host_ms=round(h_ms, 3), host_iters=h_res.n_iter, same_items=list(d_res[0]) == list(h_res[0]),
                           speedup=round(h_ms / d_ms, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "runs": a.runs, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
