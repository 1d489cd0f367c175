"""Loading and saving trained parameters (include/rmx.h "loading and saving parameters", csrc/param_io.hip,
rmx/checkpoint.py): row ranges into and out of a table, a shard and an optimiser's state, and checkpoints.

Every comparison is np.array_equal on raw fp32 values.  Expected rows come from the oracle's generator
(oracle_ctypes.gen_table, round_bf16 for bf16 tables), never from the code under test.

V = 50,003: no multiple of any N used and no perfect square, so the Feistel walk cycles and the last partition is
short.  io_chunk_rows = 4,096 here, so V spans 13 chunks: both staging buffers and a short last chunk are in play.
"""
import ctypes
import threading

import numpy as np
import pytest

import oracle_ctypes as oc
import rmx
from rmx import _lib, checkpoint
from rmx import LAYOUT_K_MAJOR as KM, LAYOUT_ROW_MAJOR as RM

pytestmark = pytest.mark.gpu

V, CHUNK = 50003, 4096
SEED = 0x51DE
F, FC, B = 5, [32, 32], 257
OTHER_KEY = 0x1234ABCD5678
HYPER = {"sgd": dict(eta=0.05), "momentum": dict(eta=0.05), "adagrad": dict(eta=0.05), "adam": dict(eta=0.01)}
NSLOTS = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}


@pytest.fixture(autouse=True)
def _small_chunks():
    rmx.set_tuning("io_chunk_rows", CHUNK)
    yield
    rmx.set_tuning("io_chunk_rows", None)


_TABLES = {}


def host_table(k, seed=SEED, rows=V):
    """(weights [rows], embedding [rows][k]) of the oracle's generator; computed once, never written."""
    key = (k, seed, rows)
    if key not in _TABLES:
        w, e = oc.gen_table(seed, rows, k)
        w.setflags(write=False)
        e.setflags(write=False)
        _TABLES[key] = (w, e)
    return _TABLES[key]


def _run_ranks(N, fn, timeout=300):
    res, errs = [None] * N, []

    def run(r):
        try:
            res[r] = fn(r)
        except BaseException as e:  # noqa: BLE001 -- re-raised below with the rank
            errs.append((r, e))

    ts = [threading.Thread(target=run, args=(r,)) for r in range(N)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    if errs:
        raise AssertionError("rank %d failed: %r" % errs[0])
    return res


def upload_in_ranges(obj, w, e, cuts, kmajor=(1,)):
    """Upload (w, e) into a table or shard in the ranges between `cuts`; the ranges listed in kmajor go K_MAJOR, as
    columns [a, b) of the whole [k][V] matrix (ld = V > n).  Returns the stored counts."""
    eT = np.ascontiguousarray(e.T)
    out = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if i in kmajor:
            out.append(obj.upload_rows(a, w[a:b], eT[:, a:b], KM))
        else:
            out.append(obj.upload_rows(a, w[a:b], e[a:b], RM))
    return out


def make_model(ctx, k=16, rows=V):
    m = rmx.DeepFM(rows, F, k, FC, ctx=ctx)
    m.setMats(m.initMats(0x3A75))
    m.setBias(0.01)
    return m


def make_batch(seed, rows=V, b=B):
    rng = np.random.default_rng(seed)
    return rng.integers(0, rows, b * F).astype(np.int32), (rng.random(b) > 0.6).astype(np.float32)


# ------------------------------------------------------------------ 1. table round trip ----
@pytest.mark.parametrize("k", [16, 5])
@pytest.mark.parametrize("dtype", [rmx.DTYPE_F32, rmx.DTYPE_BF16], ids=["f32", "bf16"])
def test_table_round_trip(dtype, k):
    ctx = rmx.default_context()
    w, e = host_table(k)
    want_w, want_e = (oc.round_bf16(w), oc.round_bf16(e)) if dtype == rmx.DTYPE_BF16 else (w, e)
    t = rmx.EmbeddingTable(ctx, V, k, dtype)
    try:
        # one row, a K_MAJOR range with ld > n, a range that ends one short of V, the last row; and n = 0
        upload_in_ranges(t, w, e, [0, 1, 20011, V - 1, V], kmajor=(1,))
        t.upload_rows(123, w[:0], e[:0])
        got_w, got_e = np.empty(V, np.float32), np.empty((V, k), np.float32)
        got_eT = np.empty((k, V), np.float32)
        a, b = 7001, 45002
        # other ranges than the upload's: ROW_MAJOR, K_MAJOR into columns [a, b) of a [k][V] matrix, a range ending at V
        t.download_rows(0, a, RM, got_w[:a], got_e[:a])
        t.download_rows(a, b - a, KM, got_w[a:b], got_eT[:, a:b])
        t.download_rows(b, V - b, RM, got_w[b:], got_e[b:])
        got_e[a:b] = got_eT[:, a:b].T
        assert np.array_equal(got_w, want_w)
        assert np.array_equal(got_e, want_e)
        one_w, one_e = t.download_rows(V - 1, 1)
        assert one_w[0] == want_w[V - 1] and np.array_equal(one_e[0], want_e[V - 1])
        zw, ze = t.download_rows(5, 0)
        assert zw.size == 0 and ze.size == 0
        full_w, full_eT = t.download(KM)
        assert np.array_equal(full_w, want_w) and np.array_equal(full_eT, want_e.T)
    finally:
        t.close()


def test_download_after_fill_is_the_generator():
    ctx = rmx.default_context()
    t = rmx.EmbeddingTable(ctx, V, 16)
    try:
        t.fill_synthetic(SEED)
        w, e = t.download()
        assert np.array_equal(w, host_table(16)[0]) and np.array_equal(e, host_table(16)[1])
    finally:
        t.close()


@pytest.mark.parametrize("dtype", [rmx.DTYPE_F32, rmx.DTYPE_BF16], ids=["f32", "bf16"])
def test_upload_rows_refreshes_the_line_copy(dtype):
    ctx = rmx.default_context()
    w, e = host_table(16)
    rmx.set_tuning("table_lines", 1)
    ta, tb = rmx.EmbeddingTable(ctx, V, 16, dtype), rmx.EmbeddingTable(ctx, V, 16, dtype)
    if dtype == rmx.DTYPE_BF16:  # (a bf16 table goes with a bf16 model)
        model = rmx.DeepFM(V, F, 16, FC, ctx=ctx)
        model.setPrecision(dtype)
        model.setMats(model.initMats(0x3A75))
        model.setBias(0.01)
    else:
        model = make_model(ctx)
    ids = rmx.DeviceArray.from_numpy(ctx, make_batch(7)[0])
    oa, ob = rmx.DeviceArray(ctx, B, np.float32), rmx.DeviceArray(ctx, B, np.float32)
    try:
        tb.upload(w, e)
        # first a table of other rows (the line copy is built), then the real rows by ranges: every line is rewritten
        ta.upload(w[::-1].copy(), e[::-1].copy())
        upload_in_ranges(ta, w, e, [0, 9000, 30001, V])
        model.forward_ids(ta, B, ids, oa)
        model.forward_ids(tb, B, ids, ob)
        ctx.sync()
        got, want = oa.numpy(), ob.numpy()
        assert np.all(np.isfinite(want)) and np.array_equal(got, want)
        # weights alone: the w slot of the touched lines follows
        w2 = (w[100:900] * 2).astype(np.float32)
        ta.upload_rows(100, weights=w2)
        wb = w.copy()
        wb[100:900] = w2
        tb.upload(wb, e)
        model.forward_ids(ta, B, ids, oa)
        model.forward_ids(tb, B, ids, ob)
        ctx.sync()
        assert np.array_equal(oa.numpy(), ob.numpy())
    finally:
        rmx.set_tuning("table_lines", None)
        for o in (ids, oa, ob, model, ta, tb):
            o.close()


# ------------------------------------------------------------------ 2. shard upload equals the fill ----
ODD_IDS = np.array([V, V + 5, -7, np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0, V - 1], np.int32)
CUTS = [0, 777, 31234, V]


def _gather_all(ctx, sh, k):
    ids_h = np.concatenate([np.arange(V, dtype=np.int32), ODD_IDS])
    n = len(ids_h)
    ids = rmx.DeviceArray.from_numpy(ctx, ids_h)
    gw, ge = rmx.DeviceArray(ctx, n, np.float32), rmx.DeviceArray(ctx, n * k, np.float32)
    sh.gather(ids, n, gw, ge)
    ctx.sync()
    out = (gw.numpy(), ge.numpy())
    for a in (ids, gw, ge):
        a.free()
    return out


def _shard_pair(ctx, how, key, r, groups):
    """(uploaded-to shard, filled twin) of one rank, before any rows."""
    def one(g):
        if how == "rccl1":
            return rmx.ShardedTable(ctx, V, 16, 1, 0, rmx.comm_unique_id())
        if how == "loop3":
            return rmx.ShardedTable(ctx, V, 16, 3)
        return rmx.ShardedTable(ctx, V, 16, g.nranks, r, group=g)
    pair = (one(groups[0]), one(groups[1]))
    if key is not None:
        for sh in pair:
            sh.set_owner_hash(key)
    return pair


def _upload_vs_fill(how, key, r, groups):
    ctx = rmx.Context(0) if groups[0] is not None else rmx.default_context()
    w, e = host_table(16)
    sh, twin = _shard_pair(ctx, how, key, r, groups)
    model = make_model(ctx)
    ids = rmx.DeviceArray.from_numpy(ctx, make_batch(11 + r)[0])
    oa, ob = rmx.DeviceArray(ctx, B, np.float32), rmx.DeviceArray(ctx, B, np.float32)
    try:
        stored = upload_in_ranges(sh, w, e, CUTS, kmajor=(1,))
        twin.fill_synthetic(SEED)
        got, want = _gather_all(ctx, sh, 16), _gather_all(ctx, twin, 16)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(want[0][:V], w) and not np.any(want[0][V:V + 5])  # the twin itself is the generator
        model.forward_ids_sharded(sh, B, ids, oa)
        model.forward_ids_sharded(twin, B, ids, ob)
        ctx.sync()
        assert np.all(np.isfinite(ob.numpy())) and np.array_equal(oa.numpy(), ob.numpy())
        _, _, owned = sh.download_rows(CUTS[1], CUTS[2] - CUTS[1])
        return stored, owned
    finally:
        for o in (ids, oa, ob, model, sh, twin):
            o.close()
        if groups[0] is not None:
            ctx.close()


@pytest.mark.parametrize("key", [None, 0], ids=["defaultkey", "key0"])
@pytest.mark.parametrize("how", ["loop3", "group2", "group4", "rccl1"])
def test_shard_upload_equals_the_fill(how, key):
    N = {"group2": 2, "group4": 4}.get(how)
    if N is None:
        stored, owned = _upload_vs_fill(how, key, 0, (None, None))
        assert stored == [b - a for a, b in zip(CUTS[:-1], CUTS[1:])] and owned.all()
        return
    groups = (rmx.ExchangeGroup(N), rmx.ExchangeGroup(N))
    try:
        res = _run_ranks(N, lambda r: _upload_vs_fill(how, key, r, groups))
    finally:
        for g in groups:
            g.close()
    for i, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        per = [res[r][0][i] for r in range(N)]
        assert sum(per) == b - a and (b - a < 4 * N or all(per)), per
    masks = np.stack([res[r][1] for r in range(N)])
    assert np.array_equal(masks.sum(0), np.ones(CUTS[2] - CUTS[1], np.int64))  # disjoint, and they cover the range


# ------------------------------------------------------------------ 3. partial and missing rows ----
@pytest.mark.parametrize("how", ["loop3", "rccl1"])
def test_partial_and_missing_rows(how):
    ctx = rmx.default_context()
    w, e = host_table(16)
    sh = (rmx.ShardedTable(ctx, V, 16, 3) if how == "loop3"
          else rmx.ShardedTable(ctx, V, 16, 1, 0, rmx.comm_unique_id()))
    model = make_model(ctx)
    ids_h = make_batch(5)[0]
    ids = rmx.DeviceArray.from_numpy(ctx, ids_h)
    out = rmx.DeviceArray(ctx, B, np.float32)
    a, b = 1000, 30000
    try:
        assert sh.upload_rows(a, w[a:b], e[a:b]) == b - a
        want_w, want_e = np.zeros(V, np.float32), np.zeros((V, 16), np.float32)
        want_w[a:b], want_e[a:b] = w[a:b], e[a:b]
        gw, ge, owned = sh.download_rows(0, V)
        assert owned.all() and np.array_equal(gw, want_w) and np.array_equal(ge, want_e)  # never uploaded: zeros
        aw, ae = _gather_all(ctx, sh, 16)
        assert np.array_equal(aw[:V], want_w) and np.array_equal(ae[:V * 16].reshape(V, 16), want_e)
        assert not np.any(aw[V:V + 5]) and not np.any(ae[V * 16:(V + 5) * 16])  # ids outside the table: zero rows
        # weights alone leave the embedding bits, embeddings alone the weight bits
        w2 = (w[5000:6000] + 1).astype(np.float32)
        sh.upload_rows(5000, weights=w2)
        want_w[5000:6000] = w2
        e2 = (e[7000:7100] * 3).astype(np.float32)
        sh.upload_rows(7000, embedding=e2)
        want_e[7000:7100] = e2
        gw, ge, _ = sh.download_rows(0, V)
        assert np.array_equal(gw, want_w) and np.array_equal(ge, want_e)
        with pytest.raises(rmx.IllegalArgumentError):
            sh.set_owner_hash(77)  # the rows are placed: the owner function is fixed
        # a pending pull: refused, and nothing moved; fine again once the slot is consumed
        sh.pull(ids, len(ids_h), 0)
        with pytest.raises(rmx.IllegalArgumentError) as ei:
            sh.upload_rows(0, w[:10], e[:10])
        assert ei.value.code == _lib.RMX_E_INVALID and "slot" in str(ei.value)
        with pytest.raises(rmx.IllegalArgumentError):
            sh.download_rows(0, 10)
        model.forward_pulled(sh, B, 0, out)
        ctx.sync()
        assert sh.upload_rows(0, w[:10], e[:10]) == 10
        want_w[:10], want_e[:10] = w[:10], e[:10]
        gw, ge, _ = sh.download_rows(0, V)
        assert np.array_equal(gw, want_w) and np.array_equal(ge, want_e)
    finally:
        for o in (ids, out, model, sh):
            o.close()


# ------------------------------------------------------------------ training helpers ----
def download_all(obj, cuts=(0, 12345, 40000, V)):
    """(weights, embedding) of a table, or (weights, embedding, owned) of a shard, read in several ranges."""
    parts = [obj.download_rows(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(len(parts[0])))


def state_all(opt, cuts=(0, 20001, V)):
    out = []
    for slot in range(opt.nslots):
        parts = [opt.state_download_rows(slot, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        out.append(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)))
    return out


def merge(per_rank):
    """The masked merge of the ranks' (weights, embedding, owned): every row from the rank that owns it."""
    masks = np.stack([p[2] for p in per_rank])
    assert np.array_equal(masks.sum(0), np.ones(masks.shape[1], np.int64))
    w, e = np.zeros_like(per_rank[0][0]), np.zeros_like(per_rank[0][1])
    for pw, pe, own in per_rank:
        w[own], e[own] = pw[own], pe[own]
    return w, e


def snapshot(model, obj, opt):
    return dict(rows=download_all(obj), state=state_all(opt), mats=model.getMats(), bias=np.float32(model.getBias()),
                dense=[opt.state_download_dense(s) for s in range(opt.nslots)], steps=opt.steps)


def assert_snap_equal(got, want, what, merged=False):
    """Two snapshots agree to the last bit (merged: both already hold (weights, embedding) pairs)."""
    for i in range(2):
        assert np.array_equal(got["rows"][i], want["rows"][i]), (what, "rows", i)
    assert len(got["state"]) == len(want["state"]), what
    for s, (a, b) in enumerate(zip(got["state"], want["state"])):
        for i in range(2):
            assert np.array_equal(a[i], b[i]), (what, "state", s, i)
    assert np.array_equal(got["mats"], want["mats"]) and got["bias"] == want["bias"], what
    for (am, ab), (bm, bb) in zip(got["dense"], want["dense"]):
        assert np.array_equal(am, bm) and np.float32(ab) == np.float32(bb), what
    assert got["steps"] == want["steps"], what


def merged_snapshot(per_rank):
    """One snapshot from the ranks' (rank order): rows and state merged by ownership; the replicas' dense parts
    must already agree."""
    out = dict(per_rank[0])
    out["rows"] = merge([p["rows"] for p in per_rank])
    out["state"] = [merge([p["state"][s] for p in per_rank]) for s in range(len(per_rank[0]["state"]))]
    for p in per_rank[1:]:
        assert np.array_equal(p["mats"], out["mats"]) and p["bias"] == out["bias"] and p["steps"] == out["steps"]
    return out


def twin_steps(opt_kind, batches):
    """A replicated twin trained by apply() on the ranks' batches concatenated in rank order (the sharded summation
    contract, tests/test_shard_optim.py): batches[step][rank] = (ids, targets).  Returns its snapshot."""
    ctx = rmx.default_context()
    model = make_model(ctx)
    table = rmx.EmbeddingTable(ctx, V, 16)
    table.fill_synthetic(SEED)
    opt = rmx.Optimizer(model, table, opt_kind, **HYPER[opt_kind])
    n_mats = model.matsLength()
    up = lambda x: rmx.DeviceArray.from_numpy(ctx, x)
    try:
        for per_rank in batches:
            grads = []
            for ids_h, tg_h in per_rank:
                n = len(ids_h)
                ids, tg = up(ids_h), up(tg_h)
                g = [up(np.zeros(m, np.float32)) for m in (1, n, n * 16, n_mats, 1)]
                model.backward_ids(table, len(tg_h), ids, tg, *g)
                ctx.sync()
                grads.append([ids_h] + [x.numpy() for x in g[:4]])
                for x in [ids, tg] + g:
                    x.free()
            g_b, g_m = grads[0][1].copy(), grads[0][4].copy()
            for d in grads[1:]:
                g_b, g_m = (g_b + d[1]).astype(np.float32), (g_m + d[4]).astype(np.float32)
            cat = lambda i: np.concatenate([d[i] for d in grads])
            arrs = [up(cat(0)), up(g_b), up(cat(2)), up(cat(3)), up(g_m)]
            opt.apply(len(cat(0)) // F, *arrs)
            ctx.sync()
            for x in arrs:
                x.free()
        return snapshot(model, table, opt)
    finally:
        for o in (opt, table, model):
            o.close()


def group_run(N, opt_kind, batches, between=None, key=None):
    """Train a group shard over batches[step][rank]; between(r, model, sh, opt) may replace the objects after a
    step (it returns (model, sh, opt, ctx) or None).  Returns per rank (losses, snapshot)."""
    g = rmx.ExchangeGroup(N)

    def rank(r):
        ctx = rmx.Context(0)
        sh = rmx.ShardedTable(ctx, V, 16, N, r, group=g)
        if key is not None:
            sh.set_owner_hash(key)
        sh.fill_synthetic(SEED)
        model = make_model(ctx)
        opt = rmx.Optimizer(model, sh, opt_kind, **HYPER[opt_kind])
        losses = []
        try:
            for step, per_rank in enumerate(batches):
                ids_h, tg_h = per_rank[r]
                ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
                losses.append(np.float32(model.train_step_sharded(sh, opt, len(tg_h), ids, tg)))
                ids.free()
                tg.free()
                if between is not None:
                    new = between(r, step, ctx, model, sh, opt)
                    if new is not None:
                        ctx, model, sh, opt = new
            return losses, snapshot(model, sh, opt)
        finally:
            for o in (opt, sh, model, ctx):
                o.close()

    try:
        return _run_ranks(N, rank)
    finally:
        g.close()


# ------------------------------------------------------------------ 4. download after training ----
def test_download_after_group_training_equals_the_replicated_twin():
    N = 2
    batches = [[make_batch(300 + 10 * s + r, b=(B, 200)[r]) for r in range(N)] for s in range(3)]
    want = twin_steps("adam", batches)
    res = group_run(N, "adam", batches)
    got = merged_snapshot([res[r][1] for r in range(N)])
    assert np.any(want["state"][1][1] != 0) and not np.array_equal(want["rows"][1], host_table(16)[1])
    assert_snap_equal(got, want, "group N=2")


def test_download_after_loopback_training_equals_the_replicated_twin():
    ctx = rmx.default_context()
    ma, mb = make_model(ctx), make_model(ctx)
    table, sh = rmx.EmbeddingTable(ctx, V, 16), rmx.ShardedTable(ctx, V, 16, 3)
    table.fill_synthetic(SEED)
    sh.fill_synthetic(SEED)
    oa, ob = rmx.Optimizer(ma, sh, "adam", **HYPER["adam"]), rmx.Optimizer(mb, table, "adam", **HYPER["adam"])
    try:
        for s in range(3):
            ids_h, tg_h = make_batch(400 + s)
            ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
            la, lb = ma.train_step_sharded(sh, oa, B, ids, tg), mb.train_step_ids(table, ob, B, ids, tg)
            assert np.float32(la) == np.float32(lb)
            ids.free()
            tg.free()
        got, want = snapshot(ma, sh, oa), snapshot(mb, table, ob)
        assert got["rows"][2].all() and all(s[2].all() for s in got["state"])
        assert np.any(want["state"][0][0] != 0) and np.any(want["state"][1][1] != 0)
        assert_snap_equal(got, want, "loopback N=3")
    finally:
        for o in (oa, ob, sh, table, ma, mb):
            o.close()


# ------------------------------------------------------------------ 5. resume is bitwise ----
def _table_run(opt_kind, batches, stop=None, path=None, forget_steps=False):
    """Losses and per-step snapshots of train_step_ids over the batches; with stop: save after `stop` steps, close
    everything, load into new objects and go on (forget_steps: with the step count left at 0)."""
    ctx = rmx.default_context()

    def fresh(fill):
        model = make_model(ctx)
        table = rmx.EmbeddingTable(ctx, V, 16)
        if fill:
            table.fill_synthetic(SEED)
        return model, table, rmx.Optimizer(model, table, opt_kind, **HYPER[opt_kind])

    model, table, opt = fresh(True)
    losses, snaps = [], []
    try:
        for step, (ids_h, tg_h) in enumerate(batches):
            if stop is not None and step == stop:
                checkpoint.save(path, model, table, opt, chunk_rows=10000)
                for o in (opt, table, model):
                    o.close()
                model, table, opt = fresh(False)
                model.setMats(np.zeros(model.matsLength(), np.float32))  # nothing survives but the checkpoint
                checkpoint.load(path, model, table, opt, chunk_rows=7001)
                if forget_steps:
                    opt.steps = 0
            ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
            losses.append(np.float32(model.train_step_ids(table, opt, len(tg_h), ids, tg)))
            ids.free()
            tg.free()
            snaps.append(snapshot(model, table, opt))
        return losses, snaps
    finally:
        for o in (opt, table, model):
            o.close()


@pytest.mark.parametrize("opt_kind", ["sgd", "momentum", "adagrad", "adam"])
def test_resume_is_bitwise_on_a_table(opt_kind, tmp_path):
    batches = [make_batch(500 + s) for s in range(5)]
    l_ref, s_ref = _table_run(opt_kind, batches)
    l_res, s_res = _table_run(opt_kind, batches, stop=3, path=str(tmp_path / "ck"))
    assert l_res[3] == l_ref[3] and l_res[4] == l_ref[4] and np.isfinite(l_ref[4])
    assert s_res[4]["steps"] == 5 and len(s_ref[4]["state"]) == NSLOTS[opt_kind]
    for step in (3, 4):
        assert_snap_equal(s_res[step], s_ref[step], "%s step %d" % (opt_kind, step + 1))
    meta = checkpoint.read_meta(str(tmp_path / "ck"))
    assert meta["optimizer"]["steps"] == 3 and meta["V"] == V and meta["model"]["fcDims"] == FC
    if opt_kind == "adam":  # a load that forgets t must not pass: Adam's bias correction differs at t = 1
        _, s_bad = _table_run(opt_kind, batches[:4], stop=3, path=str(tmp_path / "ck2"), forget_steps=True)
        assert not np.array_equal(s_bad[3]["mats"], s_ref[3]["mats"])
        assert not np.array_equal(s_bad[3]["rows"][1], s_ref[3]["rows"][1])


def test_resume_is_bitwise_on_a_group_shard(tmp_path):
    N, path = 2, str(tmp_path / "ck")
    batches = [[make_batch(600 + 10 * s + r, b=(B, 200)[r]) for r in range(N)] for s in range(5)]
    ref = group_run(N, "adam", batches)
    g2, bar = rmx.ExchangeGroup(N), threading.Barrier(N)

    def between(r, step, ctx, model, sh, opt):
        if step != 2:
            return None
        if r == 0:
            checkpoint.prepare(path, model, sh, opt)
        bar.wait(120)
        checkpoint.save(path, model, sh, opt, chunk_rows=10000, create=False)
        bar.wait(120)
        for o in (opt, sh, model, ctx):
            o.close()
        ctx = rmx.Context(0)
        sh = rmx.ShardedTable(ctx, V, 16, N, r, group=g2)
        model = rmx.DeepFM(V, F, 16, FC, ctx=ctx)
        opt = rmx.Optimizer(model, sh, "adam", **HYPER["adam"])
        checkpoint.load(path, model, sh, opt, chunk_rows=7001)
        return ctx, model, sh, opt

    try:
        res = group_run(N, "adam", batches, between=between)
    finally:
        g2.close()
    for r in range(N):
        assert res[r][0][3:] == ref[r][0][3:], ("losses", r)
    got, want = merged_snapshot([x[1] for x in res]), merged_snapshot([x[1] for x in ref])
    assert want["steps"] == 5 and np.any(want["state"][1][1] != 0)
    assert_snap_equal(got, want, "group resume")


# ------------------------------------------------------------------ 6. re-sharding ----
def test_a_group_checkpoint_loads_into_another_sharding(tmp_path):
    N, path = 2, str(tmp_path / "ck")
    batches = [[make_batch(700 + 10 * s + r, b=(B, 200)[r]) for r in range(N)] for s in range(2)]
    bar = threading.Barrier(N)

    def between(r, step, ctx, model, sh, opt):
        if step == 1:
            if r == 0:
                checkpoint.prepare(path, model, sh, opt)
            bar.wait(120)
            checkpoint.save(path, model, sh, opt, chunk_rows=9999, create=False)
            bar.wait(120)
        return None

    res = group_run(N, "adam", batches, between=between)
    want = merged_snapshot([x[1] for x in res])
    ctx = rmx.default_context()
    sh = rmx.ShardedTable(ctx, V, 16, 3)
    sh.set_owner_hash(OTHER_KEY)
    model = rmx.DeepFM(V, F, 16, FC, ctx=ctx)
    opt = rmx.Optimizer(model, sh, "adam", **HYPER["adam"])
    try:
        checkpoint.load(path, model, sh, opt)
        got = snapshot(model, sh, opt)
        assert got["rows"][2].all()
        assert_snap_equal(got, want, "N=2 -> loopback N=3, another key")
        assert np.array_equal(np.load(path + "/embedding.npy"), want["rows"][1])  # global-id indexed on disk
        assert np.array_equal(np.load(path + "/s1_weights.npy"), want["state"][1][0])
    finally:
        for o in (opt, sh, model):
            o.close()


# ------------------------------------------------------------------ 7. scratch is bounded and owned ----
def test_scratch_is_bounded_and_owned():
    ctx = rmx.default_context()
    k = 16
    start = rmx.debug_live_device_memory()
    chunk_bytes = 2 * CHUNK * (4 * k + 4 + 1) + 8  # two chunks of rows, weights and owned flags; the stored count
    objs = []
    try:
        for rows, make in ((V, lambda: rmx.EmbeddingTable(ctx, V, k)),
                           (200003, lambda: rmx.EmbeddingTable(ctx, 200003, k)),
                           (V, lambda: rmx.ShardedTable(ctx, V, k, 3))):
            w, e = host_table(k, rows=rows)
            t = make()
            objs.append(t)
            before = rmx.debug_live_device_memory()
            t.upload_rows(0, w, e)
            t.download_rows(0, rows)
            t.upload_rows(5, w[5:9000], np.ascontiguousarray(e[5:9000].T), KM)  # reused, not grown
            after = rmx.debug_live_device_memory()
            assert after[0] - before[0] == chunk_bytes, (rows, after, before)
            assert after[1] - before[1] == 7
    finally:
        for o in objs:
            o.close()
    assert rmx.debug_live_device_memory() == start


def test_row_kernels_alone_leave_the_rows_alone():
    """The bench's kernel-only hook: gets and puts of a resident chunk, both layouts; nothing changes."""
    ctx = rmx.default_context()
    w, e = host_table(16)
    table, sh = rmx.EmbeddingTable(ctx, V, 16), rmx.ShardedTable(ctx, V, 16, 3)
    try:
        for obj in (table, sh):
            obj.upload_rows(0, w, e)
            for layout, id0, n in ((RM, 0, CHUNK), (KM, V - 1000, 1000)):
                g, p = rmx.debug_row_kernels(obj, id0, n, 3, layout)
                assert g > 0 and p > 0
            with pytest.raises(rmx.IllegalArgumentError):
                rmx.debug_row_kernels(obj, 0, CHUNK + 1, 3)
            got = obj.download_rows(0, V)
            assert np.array_equal(got[0], w) and np.array_equal(got[1], e)
    finally:
        sh.close()
        table.close()


# ------------------------------------------------------------------ 8. misuse ----
def _raw(fn, *args):
    return fn(*args), (_lib.lib.rmx_last_error() or b"").decode()


def test_misuse_returns_its_code_and_touches_nothing():
    ctx = rmx.default_context()
    w, e = host_table(16)
    L = _lib.lib
    table, sh = rmx.EmbeddingTable(ctx, V, 16), rmx.ShardedTable(ctx, V, 16, 3)
    models = {"deepfm": make_model(ctx), "lr": rmx.LR(V, F, ctx=ctx),
              "dnn": rmx.DNN(V, F, 16, FC, ctx=ctx)}
    models["lr"].setBias(0.0)
    models["dnn"].setMats(models["dnn"].initMats(3))
    models["dnn"].setBias(0.0)
    opts = {"momentum": rmx.Optimizer(models["deepfm"], table, "momentum", eta=0.1),
            "sgd": rmx.Optimizer(models["deepfm"], table, "sgd", eta=0.1),
            "lr": rmx.Optimizer(models["lr"], table, "adam", eta=0.1),
            "dnn": rmx.Optimizer(models["dnn"], table, "adam", eta=0.1)}
    buf_w, buf_e = np.full(64, 9.0, np.float32), np.full(64 * 16, 9.0, np.float32)
    pw, pe = ctypes.c_void_p(buf_w.ctypes.data), ctypes.c_void_p(buf_e.ctypes.data)
    INV, IDX = _lib.RMX_E_INVALID, _lib.RMX_E_INDEX
    try:
        table.upload(w, e)
        sh.upload_rows(0, w, e)
        before = (table.download(), sh.download_rows(0, V), state_all(opts["momentum"]))
        bad = [  # (n, id0, layout, ld) -> code, the argument named
            ((-1, 0, RM, 0), INV, "n"), ((8, 0, 7, 0), INV, "layout"), ((8, 0, KM, 7), INV, "ld"),
            ((8, -1, RM, 0), IDX, "id0"), ((8, V - 7, RM, 0), IDX, "id0"), ((1, V, KM, 1), IDX, "id0")]
        for (n, id0, lay, ld), code, name in bad:
            calls = [(L.rmx_table_upload_rows, (table.handle, id0, n, pw, pe, lay, ld)),
                     (L.rmx_table_download_rows, (table.handle, id0, n, pw, pe, lay, ld)),
                     (L.rmx_shard_upload_rows, (sh.handle, id0, n, pw, pe, lay, ld, None)),
                     (L.rmx_shard_download_rows, (sh.handle, id0, n, pw, pe, lay, ld, None, None)),
                     (L.rmx_optim_state_upload_rows, (opts["momentum"].handle, 0, id0, n, pw, pe, lay, ld, None)),
                     (L.rmx_optim_state_download_rows,
                      (opts["momentum"].handle, 0, id0, n, pw, pe, lay, ld, None, None))]
            for fn, args in calls:
                st, msg = _raw(fn, *args)
                assert st == code and name in msg, (fn.__name__, n, id0, lay, ld, st, msg)
        # slots and parts an optimiser does not have
        for o, slot, a, b in ((opts["momentum"], 1, pw, pe), (opts["sgd"], 0, pw, pe), (opts["momentum"], -1, pw, pe),
                              (opts["lr"], 0, None, pe), (opts["dnn"], 0, pw, None)):
            for fn, tail in ((L.rmx_optim_state_upload_rows, (None,)), (L.rmx_optim_state_download_rows, (None, None))):
                st, msg = _raw(fn, o.handle, slot, 0, 8, a, b, RM, 0, *tail)
                assert st == INV and msg, (fn.__name__, slot, msg)
        assert _raw(L.rmx_optim_state_upload_dense, opts["sgd"].handle, 0, None, pw)[0] == INV
        assert _raw(L.rmx_optim_state_download_dense, opts["momentum"].handle, 1, None, pw)[0] == INV
        assert _raw(L.rmx_optim_set_steps, opts["sgd"].handle, -1)[0] == INV and opts["sgd"].steps == 0
        # the good halves of LR / DNN state do work
        assert L.rmx_optim_state_download_rows(opts["lr"].handle, 0, 0, 8, pw, None, RM, 0, None, None) == 0
        assert L.rmx_optim_state_download_rows(opts["dnn"].handle, 1, 0, 8, None, pe, RM, 0, None, None) == 0
        assert not np.any(buf_w[:8]) and not np.any(buf_e[:128]) and np.all(buf_w[8:] == 9) and np.all(buf_e[128:] == 9)
        after = (table.download(), sh.download_rows(0, V), state_all(opts["momentum"]))
        for x, y in zip(before[:2], after[:2]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        assert all(np.array_equal(p, q) for s, t in zip(before[2], after[2]) for p, q in zip(s, t))
        assert np.array_equal(after[0][1], e)
    finally:
        for o in list(opts.values()) + [sh, table] + list(models.values()):
            o.close()
