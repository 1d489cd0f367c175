#!/usr/bin/env python3
"""Times the device optimiser step: ms per Optimizer.apply and per train_step_ids for DeepFM 400^3, F = 39,
k = 16, V = 1M, B = 65,536, with uniform and Zipf-1.1 ids, SGD and Adam, and the backward alone in the same
process.  Prints one JSON line.

Every (ids, optimiser) case runs in a child process of its own under a time limit; after a case that fails or
runs out of time nothing more is started.

    python recommendation-models_amd/tools/bench_optim.py [--iters 20] [--warmup 3] [--timeout 240]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

F, K, V, B = 39, 16, 1_000_000, 65_536
FC = [400, 400, 400]
HBM_TBPS = 5.0  # the rate the byte model is priced at


def byte_model(nnz, distinct, slots, passes):
    """Unmeasured traffic model of one apply: the gradient rows read once, the grouping passes (8-B pairs read and
    written, keys read once more for the histogram), and every touched row's parameters and state read and written."""
    grad = nnz * (K + 1) * 4
    group = nnz * passes * (8 + 8 + 4)
    rows = distinct * (2 + 2 * slots) * (K + 1) * 4
    return dict(grad_bytes=grad, grouping_bytes=group, row_bytes=rows, total_bytes=grad + group + rows,
                model_ms=(grad + group + rows) / (HBM_TBPS * 1e12) * 1e3)


def child(dist, opt_kind, iters, warmup):
    import numpy as np
    import rmx
    ctx = rmx.default_context()
    model = rmx.DeepFM(V, F, K, FC, ctx=ctx)
    model.setMats(model.initMats(11))
    model.setBias(0.01)
    table = rmx.EmbeddingTable(ctx, V, K)
    table.fill_synthetic(7)
    ids = rmx.DeviceArray(ctx, B * F, np.int32)
    rmx.gen_ids(ctx, 5, 0, B, F, V, ids, zipf=1.1 if dist == "zipf" else 0.0)
    ctx.sync()
    ids_h = ids.numpy()
    _, counts = np.unique(ids_h, return_counts=True)
    targets = rmx.DeviceArray.from_numpy(ctx, (np.random.default_rng(3).random(B) > 0.7).astype(np.float32))
    nnz = B * F
    g_b, g_w = rmx.DeviceArray(ctx, 1, np.float32), rmx.DeviceArray(ctx, nnz, np.float32)
    g_e, g_m = rmx.DeviceArray(ctx, nnz * K, np.float32), rmx.DeviceArray(ctx, model.matsLength(), np.float32)
    loss = rmx.DeviceArray(ctx, 1, np.float32)
    opt = rmx.Optimizer(model, table, opt_kind, eta=1e-4)
    ev = [ctypes_event() for _ in range(2)]

    def timed_async(fn):
        """ms per call of an asynchronous call, by events around `iters` back-to-back calls"""
        for _ in range(warmup):
            fn()
        ctx.sync()
        rmx._lib.check(rmx._lib.lib.rmx_event_record(ev[0], ctx.stream))
        for _ in range(iters):
            fn()
        rmx._lib.check(rmx._lib.lib.rmx_event_record(ev[1], ctx.stream))
        ms = ctypes.c_float()
        rmx._lib.check(rmx._lib.lib.rmx_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value / iters

    def timed_sync(fn):
        """ms per call of a call that synchronises, by the host clock"""
        for _ in range(warmup):
            fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / iters

    res = dict(ids=dist, optimizer=opt_kind, distinct_ids=int(len(counts)), max_occurrences=int(counts.max()),
               lists_over_512=int((counts > 512).sum()))
    res["backward_ms"] = timed_async(lambda: model.backward_ids(table, B, ids, targets, g_b, g_w, g_e, g_m, loss))
    # the gradients of the last backward, applied over and over (eta is tiny: the values stay finite)
    res["apply_table_ms"] = timed_async(lambda: opt.apply(B, ids, None, g_w, g_e, None))
    res["apply_ms"] = timed_sync(lambda: opt.apply(B, ids, g_b, g_w, g_e, g_m))
    res["train_step_ms"] = timed_sync(lambda: model.train_step_ids(table, opt, B, ids, targets))
    slots = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}[opt_kind]
    passes = (int(V).bit_length() + 7) // 8
    res["byte_model"] = byte_model(nnz, res["distinct_ids"], slots, passes)
    res["apply_over_model"] = res["apply_ms"] / res["byte_model"]["model_ms"]
    res["apply_over_backward"] = res["apply_ms"] / res["backward_ms"]
    print("RESULT " + json.dumps(res), flush=True)
    opt.close()
    rmx.shutdown()


def ctypes_event():
    import rmx
    e = ctypes.c_void_p()
    rmx._lib.check(rmx._lib.lib.rmx_event_create(ctypes.byref(e)))
    return e



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", nargs=2, metavar=("IDS", "OPT"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup)
        return 0
    out = dict(bench="optim", model="deepfm", fc=FC, F=F, k=K, V=V, B=B, iters=a.iters, cases=[])
    for dist in ("uniform", "zipf"):
        for opt_kind in ("sgd", "adam"):
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--warmup", str(a.warmup),
                   "--child", dist, opt_kind]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                out["error"] = "case %s/%s ran out of time (%d s); nothing more was started" % (dist, opt_kind, a.timeout)
                print(json.dumps(out))
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                out["error"] = "case %s/%s failed with status %d: %s" % (dist, opt_kind, p.returncode,
                                                                         p.stderr.strip()[-400:])
                print(json.dumps(out))
                return 1
            out["cases"].append(json.loads(line[-1][len("RESULT "):]))
    by = {(c["ids"], c["optimizer"]): c for c in out["cases"]}
    out["zipf_over_uniform"] = {o: by[("zipf", o)]["apply_ms"] / by[("uniform", o)]["apply_ms"] for o in ("sgd", "adam")}
    out["zipf_over_uniform_table"] = {o: by[("zipf", o)]["apply_table_ms"] / by[("uniform", o)]["apply_table_ms"]
                                      for o in ("sgd", "adam")}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
