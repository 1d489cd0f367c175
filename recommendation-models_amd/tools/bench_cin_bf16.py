#!/usr/bin/env python3
"""Times the xDeepFM forward with the fp32 CIN against the bf16 CIN (setCinPrecision(DTYPE_BF16)) in ONE process:
an fp32 model and a bf16-CIN model of the same mats alternate on the same table and ids.  F = 39, k = 16,
fc 400^3, V = 1M; CIN (200, 200, 200) and the reference-exact (200,); B = 4,096 and 65,536.  Per case: warm-up,
then `passes` alternating passes, each of `iters` timed forwards per arm (events around the back-to-back calls)
and `iters` more with the stage timers on (rmx_model_get_timing: cin_layer1 / 2 / 3+).  Prints one JSON line: per
arm the ms per forward of every pass, their median and spread, the per-stage ms (median over the passes, and the
spread between them), and max |p_bf16 - p_fp32|.

    python recommendation-models_amd/tools/bench_cin_bf16.py [--iters 20] [--warmup 3] [--passes 3]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

F, K, V = 39, 16, 1_000_000
FC = [400, 400, 400]
CINS = ([200, 200, 200], [200])
BATCHES = (4096, 65536)
ARMS = ("f32", "bf16_cin")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    if a.passes < 3:
        ap.error("--passes must be at least 3")
    import numpy as np
    import rmx
    lib, check = rmx._lib.lib, rmx._lib.check
    ctx = rmx.default_context()
    table = rmx.EmbeddingTable(ctx, V, K)
    table.fill_synthetic(7)
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        check(lib.rmx_event_create(ctypes.byref(e)))

    def timed(fn, n):
        check(lib.rmx_event_record(ev[0], ctx.stream))
        for _ in range(n):
            fn()
        check(lib.rmx_event_record(ev[1], ctx.stream))
        ms = ctypes.c_float()
        check(lib.rmx_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value / n

    out = dict(bench="cin_bf16", model="xdeepfm", fc=FC, F=F, k=K, V=V, iters=a.iters, warmup=a.warmup,
               passes=a.passes, cases=[])
    for cin in CINS:
        models = {}
        for arm in ARMS:
            m = rmx.XDeepFM(V, F, K, FC, cin, ctx=ctx)
            if arm == "bf16_cin":
                m.setCinPrecision(rmx.DTYPE_BF16)
            m.setMats(m.initMats(11))
            m.setBias(0.01)
            models[arm] = m
        for B in BATCHES:
            ids = rmx.DeviceArray(ctx, B * F, np.int32)
            rmx.gen_ids(ctx, 5, 0, B, F, V, ids)
            outs = {arm: rmx.DeviceArray(ctx, B, np.float32) for arm in ARMS}
            run = {arm: (lambda arm=arm: models[arm].forward_ids(table, B, ids, outs[arm])) for arm in ARMS}
            for arm in ARMS:
                for _ in range(a.warmup):
                    run[arm]()
            ctx.sync()
            ms = {arm: [] for arm in ARMS}
            st = {arm: [] for arm in ARMS}
            for _ in range(a.passes):
                for arm in ARMS:
                    ms[arm].append(timed(run[arm], a.iters))
                    m = models[arm]
                    m.set_timing(True)
                    for _ in range(a.iters):
                        run[arm]()
                    ctx.sync()
                    stages, calls = m.get_timing()
                    m.set_timing(False)
                    st[arm].append({k_: v / max(calls, 1) for k_, v in stages.items()})
            case = dict(cin=cin, B=B)
            for arm in ARMS:
                med = statistics.median(ms[arm])
                names = list(st[arm][0])
                case[arm] = dict(ms_per_forward=med, passes_ms=ms[arm], spread_ms=max(ms[arm]) - min(ms[arm]),
                                 examples_per_s=B / med * 1e3,
                                 stage_ms={s: statistics.median(p_[s] for p_ in st[arm]) for s in names},
                                 stage_spread_ms={s: max(p_[s] for p_ in st[arm]) - min(p_[s] for p_ in st[arm])
                                                  for s in names})
            ctx.sync()
            case["max_abs_dp"] = float(np.abs(outs["bf16_cin"].numpy() - outs["f32"].numpy()).max())
            case["speedup"] = case["f32"]["ms_per_forward"] / case["bf16_cin"]["ms_per_forward"]
            case["cin_stage_ratio"] = {
                s: case["f32"]["stage_ms"][s] / case["bf16_cin"]["stage_ms"][s]
                for s in case["f32"]["stage_ms"] if s.startswith("cin_layer") and case["bf16_cin"]["stage_ms"].get(s)}
            out["cases"].append(case)
        for m in models.values():
            m.close()
    print(json.dumps(out))
    rmx.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
