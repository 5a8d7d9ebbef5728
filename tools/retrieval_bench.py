"""Timings of the retrieval evaluation on the device (selavi_amd.retrieval_utils, csrc/retrieval.hip).

    python tools/retrieval_bench.py [--out profiles/retrieval_bench.json]

* feature extraction: clips/s of VideoRetrievalEncoder (layer 4 max-pooled 2x2x2) at 32 frames x 112^2, per feature-pass
  arithmetic;
* kNN at UCF101 split 1 (3 783 x 9 537 x 9 216) and HMDB51 split 1 (1 530 x 3 570 x 9 216): the dot-product GEMM
  (slv_gemm_nt) and the d^2 + top-50 selection (slv_knn_select) timed apart with device events, each with its floor from
  the shapes (GEMM: 2QND FLOP at 157.3 TFLOP/s fp32 MFMA; selection: the Q x N fp32 dots read once at 8 TB/s);
* the reference's sklearn NearestNeighbors path on the host, if sklearn imports (a query subset, scaled).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from selavi_amd import ops, retrieval_utils as ru  # noqa: E402
from selavi_amd._lib import C, ptr, stream  # noqa: E402
from selavi_amd.model import load_model  # noqa: E402

FP32_PEAK = 157.3e12
HBM = 8.0e12
SHAPES = {"ucf101_split1": (3783, 9537, 9216), "hmdb51_split1": (1530, 3570, 9216)}


def _events(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def bench_extraction(batch, reps):
    model = load_model(use_mlp=True, num_classes=309, headcount=10, norm_feat=False).cuda()
    x = torch.randn(batch, 3, 32, 112, 112, device="cuda")
    out = {}
    for fp in ru.FEATURE_PASSES:
        enc = ru.VideoRetrievalEncoder(model, "max", fp)
        for _ in range(2):
            enc(x)
        torch.cuda.synchronize()
        t = _events(lambda: enc(x), reps)
        out[fp] = {"clips_per_s": batch / t, "batch": batch, "ms_per_batch": t * 1e3}
    return out


def bench_knn(Q, N, D, k, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    bank = torch.nn.functional.normalize(torch.randn(N, D, device="cuda", generator=g), dim=1)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device="cuda", generator=g), dim=1)
    qs, ts = ops.row_sqnorm(q), ops.row_sqnorm(bank)
    dots = torch.empty(Q, N, device="cuda")
    d2 = torch.empty(Q, k, device="cuda")
    idx = torch.empty(Q, k, dtype=torch.int32, device="cuda")
    gemm = lambda: C.slv_gemm_nt(ptr(q), ptr(bank), 0, ptr(dots), Q, N, D, N, stream())
    sel = lambda: C.slv_knn_select(ptr(dots), N, Q, N, ptr(qs), ptr(ts), k, ptr(d2), ptr(idx), stream())
    for _ in range(2):
        gemm()
        sel()
    torch.cuda.synchronize()
    t_gemm, t_sel = _events(gemm, reps), _events(sel, reps)
    t_all = _events(lambda: ops.knn(q, bank, k), reps)
    f_gemm = 2.0 * Q * N * D / FP32_PEAK
    f_sel = 4.0 * Q * N / HBM
    return {"Q": Q, "N": N, "D": D, "k": k,
            "gemm_ms": t_gemm * 1e3, "gemm_floor_ms": f_gemm * 1e3, "gemm_tflops": 2.0 * Q * N * D / t_gemm / 1e12,
            "select_ms": t_sel * 1e3, "select_floor_ms": f_sel * 1e3,
            "knn_total_ms": t_all * 1e3}


def bench_sklearn(Q, N, D, k, n_queries):
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        return None
    g = np.random.RandomState(0)
    bank = g.randn(N, D).astype(np.float32)
    q = g.randn(n_queries, D).astype(np.float32)
    nn = NearestNeighbors(n_neighbors=k).fit(bank)
    t0 = time.perf_counter()
    for i in range(n_queries):                     # the reference: five kneighbors calls per query
        for kk in (1, 5, 10, 20, 50):
            nn.kneighbors(q[i:i + 1], kk)
    t = time.perf_counter() - t0
    return {"queries_timed": n_queries, "s_per_query": t / n_queries, "s_all_queries_est": t / n_queries * Q}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn-queries", type=int, default=20)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "measured": True}
    res["extraction_32x112"] = bench_extraction(a.batch, a.reps)
    print(json.dumps(res["extraction_32x112"]), flush=True)
    res["knn"] = {}
    for name, (Q, N, D) in SHAPES.items():
        res["knn"][name] = bench_knn(Q, N, D, 50, a.reps)
        print(name, json.dumps(res["knn"][name]), flush=True)
    res["sklearn_host"] = {name: bench_sklearn(Q, N, D, 50, a.sklearn_queries) for name, (Q, N, D) in SHAPES.items()}
    print(json.dumps(res["sklearn_host"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
