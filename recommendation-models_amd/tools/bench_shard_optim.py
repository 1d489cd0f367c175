#!/usr/bin/env python3
"""Times the training step on the sharded table: ms per train_step_sharded for DeepFM 400^3, F = 39, k = 16,
V = 1M, B = 65,536 per rank, with uniform and Zipf-1.1 ids, SGD and Adam:
  - a one-rank shard against train_step_ids on a replicated table in the same process;
  - in-process exchange groups of 2 and 4 ranks on the one GPU (one thread, context and stream per rank).  This
    records what the protocol costs -- bucketing, counts, one host sync, device copies for the exchange, the
    owner-side update.  It is NOT a scaling figure: the ranks share the device.
Beside them the unmeasured byte model of the push, nnz (k + 2) 4 (N - 1) / N bytes sent per rank, and the
train_step_ids figure recorded at the parent commit (profiles/optim/bench_optim.json) when that file is there.
Prints one JSON line and writes it to profiles/shard_optim/bench_shard_optim.json.

Every (ids, optimiser) case runs in a child process of its own under a time limit; after a case that fails or
runs out of time nothing more is started.

    python recommendation-models_amd/tools/bench_shard_optim.py [--iters 10] [--warmup 2] [--timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

F, K, V, B = 39, 16, 1_000_000, 65_536
FC = [400, 400, 400]
GROUPS = (2, 4)


def push_bytes(nnz, N):
    """Unmeasured: the bytes one rank sends to its peers in one push (local row, g_w and k g_emb floats per
    nonzero, the share of its nonzeros that other ranks own)."""
    return nnz * (K + 2) * 4 * (N - 1) // N


def child(dist, opt_kind, iters, warmup):
    import numpy as np
    import rmx

    def make(ctx):
        model = rmx.DeepFM(V, F, K, FC, ctx=ctx)
        model.setMats(model.initMats(11))
        model.setBias(0.01)
        return model

    def batch(ctx, rank):
        ids = rmx.DeviceArray(ctx, B * F, np.int32)
        rmx.gen_ids(ctx, 5, rank * B, B, F, V, ids, zipf=1.1 if dist == "zipf" else 0.0)
        tg = rmx.DeviceArray.from_numpy(ctx, (np.random.default_rng(3 + rank).random(B) > 0.7).astype(np.float32))
        ctx.sync()
        return ids, tg

    def timed(ctx, fn):
        """ms per call of a call that synchronises, by the host clock"""
        for _ in range(warmup):
            fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / iters

    nnz = B * F
    res = dict(ids=dist, optimizer=opt_kind)
    ctx = rmx.default_context()
    ids, tg = batch(ctx, 0)
    # replicated table and one-rank shard, one after the other in this process
    model = make(ctx)
    table = rmx.EmbeddingTable(ctx, V, K)
    table.fill_synthetic(7)
    opt = rmx.Optimizer(model, table, opt_kind, eta=1e-4)
    res["train_step_ids_ms"] = timed(ctx, lambda: model.train_step_ids(table, opt, B, ids, tg))
    for o in (opt, table, model):
        o.close()
    model = make(ctx)
    sh = rmx.ShardedTable(ctx, V, K, 1, 0, rmx.comm_unique_id())
    sh.fill_synthetic(7)
    opt = rmx.Optimizer(model, sh, opt_kind, eta=1e-4)
    res["train_step_sharded_1rank_ms"] = timed(ctx, lambda: model.train_step_sharded(sh, opt, B, ids, tg))
    res["sharded_1rank_over_ids"] = res["train_step_sharded_1rank_ms"] / res["train_step_ids_ms"]
    for o in (opt, sh, model):
        o.close()
    # groups: every rank steps its own batch; the ranks are in lock step, so rank 0's clock is the step's
    res["groups"] = []
    for N in GROUPS:
        g = rmx.ExchangeGroup(N)
        ms, errs = [None] * N, []

        def rank(r):
            try:
                c = rmx.Context(0)
                m = make(c)
                s = rmx.ShardedTable(c, V, K, N, r, group=g)
                s.fill_synthetic(7)
                o = rmx.Optimizer(m, s, opt_kind, eta=1e-4)
                i, t = batch(c, r)
                ms[r] = timed(c, lambda: m.train_step_sharded(s, o, B, i, t))
                for x in (o, s, m):
                    x.close()
            except BaseException as e:  # noqa: BLE001 -- reported by the parent
                errs.append("rank %d: %r" % (r, e))

        ts = [threading.Thread(target=rank, args=(r,)) for r in range(N)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        g.close()
        if errs:
            raise RuntimeError("; ".join(errs))
        res["groups"].append(dict(nranks=N, train_step_sharded_ms=ms[0], per_rank_ms=ms,
                                  examples_per_step=N * B, push_bytes_per_rank_model=push_bytes(nnz, N)))
    print("RESULT " + json.dumps(res), flush=True)
    rmx.shutdown()


def parent_figures():
    """train_step_ids ms per (ids, optimiser) as recorded before this tool existed, or {}"""
    try:
        with open(os.path.join(ROOT, "profiles", "optim", "bench_optim.json")) as f:
            return {(c["ids"], c["optimizer"]): c["train_step_ms"] for c in json.load(f)["cases"]}
    except (OSError, ValueError, KeyError):
        return {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per case")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_optim", "bench_shard_optim.json"))
    ap.add_argument("--child", nargs=2, metavar=("IDS", "OPT"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.iters, a.warmup)
        return 0
    out = dict(bench="shard_optim", model="deepfm", fc=FC, F=F, k=K, V=V, B_per_rank=B, iters=a.iters,
               note="groups share one GPU: protocol cost, not scaling", cases=[])
    before = parent_figures()
    status = 0
    for dist in ("uniform", "zipf"):
        for opt_kind in ("sgd", "adam"):
            cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--warmup", str(a.warmup),
                   "--child", dist, opt_kind]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                out["error"] = "case %s/%s ran out of time (%d s); nothing more was started" % (dist, opt_kind, a.timeout)
                status = 1
                break
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                out["error"] = "case %s/%s failed with status %d: %s" % (dist, opt_kind, p.returncode,
                                                                         p.stderr.strip()[-400:])
                status = 1
                break
            case = json.loads(line[-1][len("RESULT "):])
            case["parent_train_step_ids_ms"] = before.get((dist, opt_kind))
            out["cases"].append(case)
        if status:
            break
    print(json.dumps(out))
    if status == 0:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
