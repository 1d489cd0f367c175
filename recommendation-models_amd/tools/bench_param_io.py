#!/usr/bin/env python3
"""Times the row upload / download calls (include/rmx.h "loading and saving parameters"): GB/s of row bytes
(V * (k + 1) * 4) into and out of a replicated table and a one-rank shard, k = 16, from pageable and from pinned
host arrays; beside each figure a plain host <-> device copy of the same bytes from the same host buffer in the same
process (the bound a staging path can at best approach); and the A/Bs: io_chunk_rows over three sizes, non-temporal
against plain stores in the scatter (knob io_nt); and the gather / scatter kernels alone on a device-resident chunk
(rmx_debug_*_row_kernels), in lines per second.  Prints one JSON line.

Every target runs in a child process of its own under a time limit; after a case that fails or runs out of time
nothing more is started.

    python recommendation-models_amd/tools/bench_param_io.py [--rows 1000000] [--iters 5] [--timeout 300]
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

K = 16
CHUNKS = (65536, 262144, 1048576)


def pinned_arrays(hip, V):
    """(weights [V], embedding [V][K]) numpy views of one pinned allocation, and its pointer."""
    import numpy as np
    p = ctypes.c_void_p()
    nbytes = V * (K + 1) * 4
    if hip.hipHostMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes), 0) != 0:
        raise MemoryError("hipHostMalloc of %d bytes failed" % nbytes)
    buf = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(V * (K + 1),))
    return buf[:V], buf[V:].reshape(V, K), p


def best(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), sorted(ts)[len(ts) // 2]


def child(target, V, iters, quick):
    import numpy as np
    import rmx
    ctx = rmx.default_context()
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    obj =(rmx.EmbeddingTable(ctx, V, K) if target == "table"
           else rmx.ShardedTable(ctx, V, K, 1, 0, rmx.comm_unique_id()))
    rng = np.random.default_rng(1)
    hosts = {"pageable": (rng.random(V, np.float32), rng.random((V, K), np.float32))}
    pw, pe, pin = pinned_arrays(hip, V)
    pw[:], pe[:] = hosts["pageable"]
    hosts["pinned"] = (pw, pe)
    dev = rmx.DeviceArray(ctx, V * (K + 1), np.float32)
    gb = V * (K + 1) * 4 / 1e9
    res = dict(target=target, V=V, k=K, row_gbytes=gb, cases=[])

    def case(host, chunk, nt):
        w, e = hosts[host]
        rmx.set_tuning("io_chunk_rows", chunk)
        rmx.set_tuning("io_nt", nt)
        L = rmx._lib.lib
        up, up_med = best(lambda: obj.upload_rows(0, w, e), iters)
        down, down_med = best(lambda: obj.download_rows(0, V, weights=w, embedding=e), iters)
        # the same bytes by one plain copy each way, from / into the same host buffers
        def h2d():
            rmx._lib.check(L.rmx_memcpy_htod(ctx.handle, dev.ptr, w.ctypes.data, V * 4))
            rmx._lib.check(L.rmx_memcpy_htod(ctx.handle, ctypes.c_void_p(dev.ptr.value + V * 4), e.ctypes.data,
                                             V * K * 4))

        def d2h():
            rmx._lib.check(L.rmx_memcpy_dtoh(ctx.handle, w.ctypes.data, dev.ptr, V * 4))
            rmx._lib.check(L.rmx_memcpy_dtoh(ctx.handle, e.ctypes.data, ctypes.c_void_p(dev.ptr.value + V * 4),
                                             V * K * 4))
        c_up, _ = best(h2d, iters)
        c_down, _ = best(d2h, iters)
        res["cases"].append(dict(host=host, io_chunk_rows=chunk, io_nt=nt, upload_gbps=gb / up,
                                 upload_gbps_median=gb / up_med, download_gbps=gb / down,
                                 download_gbps_median=gb / down_med, memcpy_h2d_gbps=gb / c_up,
                                 memcpy_d2h_gbps=gb / c_down, upload_over_memcpy=c_up / up,
                                 download_over_memcpy=c_down / down))

    if quick:  # (a V = 100M run: the default chunk only)
        case("pinned", CHUNKS[1], 0)
        case("pageable", CHUNKS[1], 0)
    else:
        for host in ("pinned", "pageable"):
            for chunk in CHUNKS:
                case(host, chunk, 0)
        case("pinned", CHUNKS[1], 1)
    # the gather and the scatter kernel alone on a device-resident chunk of 1M rows (or V), in lines per second:
    # one 128-B line per row of a shard partition; a table row is a 64-B row line plus a share of a weight line
    n = min(V, CHUNKS[2])
    rmx.set_tuning("io_chunk_rows", CHUNKS[2])
    res["kernels"] = []
    for layout, lname in ((rmx.LAYOUT_ROW_MAJOR, "row_major"), (rmx.LAYOUT_K_MAJOR, "k_major")):
        for nt in (0, 1):
            rmx.set_tuning("io_nt", nt)
            g, p = rmx.debug_row_kernels(obj, 0, n, 20, layout)
            res["kernels"].append(dict(chunk_layout=lname, io_nt=nt, rows=n, get_ms=g, put_ms=p,
                                       get_glines_per_s=n / g / 1e6, put_glines_per_s=n / p / 1e6,
                                       get_gbps=gb * n / V / (g * 1e-3), put_gbps=gb * n / V / (p * 1e-3)))
    # the rows survive the trip (the last download overwrote the host arrays with what the device holds)
    assert np.array_equal(hosts["pinned"][1], hosts["pageable"][1])
    print("RESULT " + json.dumps(res), flush=True)
    rmx.set_tuning("io_chunk_rows", None)
    rmx.set_tuning("io_nt", None)
    obj.close()
    dev.free()
    hip.hipHostFree(pin)
    rmx.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per target")
    ap.add_argument("--quick", action="store_true", help="the default chunk size only (large V)")
    ap.add_argument("--targets", default="table,shard")
    ap.add_argument("--child", metavar="TARGET")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.rows, a.iters, a.quick)
        return 0
    out = dict(bench="param_io", k=K, V=a.rows, iters=a.iters, targets=[])
    for target in a.targets.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--iters", str(a.iters), "--child",
               target] + (["--quick"] if a.quick else [])
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            out["error"] = "target %s ran out of time (%d s); nothing more was started" % (target, a.timeout)
            print(json.dumps(out))
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            out["error"] = "target %s failed with status %d: %s" % (target, p.returncode, p.stderr.strip()[-400:])
            print(json.dumps(out))
            return 1
        out["targets"].append(json.loads(line[-1][len("RESULT "):]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
