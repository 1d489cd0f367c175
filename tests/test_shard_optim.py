"""Training on the sharded table (include/rmx.h rmx_backward_pulled, rmx_optim_create_sharded,
rmx_train_step_sharded; csrc/shard.hip "the push") against the replicated table.

Every comparison is np.array_equal on the raw fp32 values: the contract is bit for bit.  One sharded step over
ranks 0..N-1 must equal rmx_optim_apply on a replicated twin given the ranks' batches concatenated in rank order,
and rmx_backward_pulled must equal rmx_backward_ids on a table holding the same rows.

V = 5,003 (no multiple of any N used; small enough to gather and compare the WHOLE table every time), F = 39,
k = 16 (one case at k = 8: the optimiser's non-K16 template), towers [64, 32], CIN [48, 32]; per-rank batches
300 / 257 / 64 / 1 (ragged, more than one 4,096-element radix tile, one tiny rank).
"""
import ctypes
import threading

import numpy as np
import pytest

import rmx
from rmx import _lib

pytestmark = pytest.mark.gpu

V, F = 5003, 39
FC, CIN = [64, 32], [48, 32]
SEED_TAB, SEED_MATS = 0x7AB1E, 0x3A75
BATCHES = (300, 257, 64, 1)
NSLOTS = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}
HYPER = {"sgd": dict(eta=0.05), "momentum": dict(eta=0.05), "adagrad": dict(eta=0.05), "adam": dict(eta=0.01)}


def _run_ranks(N, fn, timeout=300):
    """fn(rank) on N threads (each rank drives its own context / stream, like N processes)."""
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


def make_model(kind, k, ctx):
    m = {"lr": lambda: rmx.LR(V, F, ctx=ctx), "deepfm": lambda: rmx.DeepFM(V, F, k, FC, ctx=ctx),
         "dnn": lambda: rmx.DNN(V, F, k, FC, ctx=ctx), "dcn": lambda: rmx.DCN(V, F, k, 3, FC, ctx=ctx),
         "pnn": lambda: rmx.PNN(V, F, k, FC, ctx=ctx),
         "xdeepfm": lambda: rmx.XDeepFM(V, F, k, FC, CIN, ctx=ctx)}[kind]()
    if kind != "lr":
        m.setMats(m.initMats(SEED_MATS))
    m.setBias(0.01)
    return m


def make_batch(seed, B):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, V, B * F).astype(np.int32), (rng.random(B) > 0.6).astype(np.float32))


def dev_read(ctx, addr, n, owner):
    if not addr:
        return None
    return rmx.DeviceArray(ctx, n, np.float32, ctypes.c_void_p(addr), owner).numpy()


def table_arrays(ctx, table):
    pw, pe = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(_lib.lib.rmx_table_device_ptrs(table.handle, ctypes.byref(pw), ctypes.byref(pe)))
    ctx.sync()
    return dev_read(ctx, pw.value, V, table), dev_read(ctx, pe.value, V * table.k, table)


def shard_arrays(ctx, sh):
    """The whole table as this rank sees it: ids 0 .. V-1 gathered from their owners (collective)."""
    ids = rmx.DeviceArray.from_numpy(ctx, np.arange(V, dtype=np.int32))
    w, e = rmx.DeviceArray(ctx, V, np.float32), rmx.DeviceArray(ctx, V * sh.k, np.float32)
    sh.gather(ids, V, w, e)
    ctx.sync()
    out = (w.numpy(), e.numpy())
    for a in (ids, w, e):
        a.free()
    return out


_OWNERS = {}


def owner_map(key, N):
    if (key, N) not in _OWNERS:
        o, l = np.empty(V, np.int64), np.empty(V, np.int64)
        for i in range(V):
            o[i], l[i] = rmx.owner_hash(key, V, N, i)
        _OWNERS[(key, N)] = (o, l)
    return _OWNERS[(key, N)]


def twin_state(ctx, opt, k, n_mats):
    """[slot] -> (w [V], emb [V * k], mats, bias) of a table's optimiser (None where it holds none)."""
    out = []
    for slot in range(2):
        p = [ctypes.c_void_p() for _ in range(4)]
        _lib.check(_lib.lib.rmx_optim_state_ptrs(opt.handle, slot, *[ctypes.byref(x) for x in p]))
        ctx.sync()
        out.append([dev_read(ctx, x.value, n, opt) for x, n in zip(p, (V, V * k, n_mats, 1))])
    return out


def shard_local_state(ctx, opt, k, rows, n_mats, parts):
    """[slot] -> ([part] -> (w [rows], emb [rows * k]), mats, bias) of a sharded optimiser."""
    out = []
    for slot in range(2):
        p = [ctypes.c_void_p() for _ in range(4)]
        _lib.check(_lib.lib.rmx_optim_state_ptrs(opt.handle, slot, *[ctypes.byref(x) for x in p]))
        assert p[0].value is None and p[1].value is None  # the table state of a shard is per partition
        ctx.sync()
        per = []
        for part in range(parts):
            aw, ae = opt.shard_state_ptrs(slot, part)
            per.append((dev_read(ctx, aw, rows, opt), dev_read(ctx, ae, rows * k, opt)))
        out.append((per, dev_read(ctx, p[2].value, n_mats, opt), dev_read(ctx, p[3].value, 1, opt)))
    return out


def assert_state_equal(parts_of_owner, twin, key, N, k, what):
    """parts_of_owner[slot][owner] = (w, emb) local arrays; twin[slot] = (w, emb, ...) over the ids."""
    own, loc = owner_map(key, N)
    for slot in range(2):
        tw, te = twin[slot][0], twin[slot][1]
        for name, t, width, idx in (("w", tw, 1, 0), ("emb", te, k, 1)):
            locs = [parts_of_owner[slot][o][idx] for o in range(N)]
            assert all((x is None) == (t is None) for x in locs), (what, slot, name)
            if t is None:
                continue
            got = np.stack([locs[o].reshape(-1, width)[l] for o, l in zip(own, loc)])
            assert np.array_equal(got, t.reshape(V, width)), (what, "state", slot, name)


class Grads:
    """Device outputs of one backward, zeroed first (a model that skips a group leaves it zero on both sides)."""

    def __init__(self, ctx, n, k, n_mats, lr):
        self.ctx = ctx
        z = lambda m: rmx.DeviceArray.from_numpy(ctx, np.zeros(max(m, 1), np.float32))
        self.g_b, self.g_w, self.loss = z(1), z(n), z(1)
        self.g_e = None if lr else z(n * k)
        self.g_m = None if lr else z(n_mats)

    def args(self):
        return (self.g_b, self.g_w, self.g_e, self.g_m, self.loss)

    def numpy(self):
        self.ctx.sync()
        return {n: (None if a is None else a.numpy()) for n, a in
                zip(("g_bias", "g_w", "g_emb", "g_mats", "loss"), self.args())}

    def free(self):
        for a in self.args():
            if a is not None:
                a.free()


def assert_same(got, ref, what):
    for name in ref:
        if ref[name] is None:
            assert got[name] is None, (what, name)
        else:
            assert np.array_equal(got[name], ref[name]), (what, name)


# ------------------------------------------------------------ 1. backward from a pull slot ----
def _shard_for(ctx, k, how):
    if how == "rccl1":  # one rank over RCCL: the direct-mapped slot (rows read in place)
        sh = rmx.ShardedTable(ctx, V, k, 1, 0, rmx.comm_unique_id())
    else:
        sh = rmx.ShardedTable(ctx, V, k, 3)
        sh.set_dedupe(how == "loop3-dedupe")
    sh.fill_synthetic(SEED_TAB)
    return sh


@pytest.mark.parametrize("how", ["loop3-dedupe", "loop3-plain", "rccl1"])
@pytest.mark.parametrize("kind", ["deepfm", "xdeepfm", "dcn", "pnn", "dnn", "lr"])
def test_backward_pulled_equals_backward_ids(kind, how):
    ctx, k, B = rmx.default_context(), 16, 300
    n = B * F
    model = make_model(kind, k, ctx)
    table = rmx.EmbeddingTable(ctx, V, k)
    table.fill_synthetic(SEED_TAB)
    sh = _shard_for(ctx, k, how)
    ids_h, tg_h = make_batch(101, B)
    ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
    ref, got = Grads(ctx, n, k, model.matsLength(), kind == "lr"), Grads(ctx, n, k, model.matsLength(), kind == "lr")
    try:
        model.backward_ids(table, B, ids, tg, *ref.args())
        sh.pull(ids, n, 0)
        model.backward_pulled(sh, B, 0, tg, *got.args())
        r, g = ref.numpy(), got.numpy()
        assert np.isfinite(r["loss"][0]) and r["loss"][0] > 0 and (kind == "dnn" or np.any(r["g_w"] != 0))
        assert_same(g, r, "%s %s" % (kind, how))
        sh.pull(ids, n, 0)  # the slot was consumed: it takes the next pull
        model.backward_pulled(sh, B, 0, tg, *got.args())
        assert_same(got.numpy(), r, "%s %s again" % (kind, how))
    finally:
        for o in (ref, got, ids, tg):
            o.free()
        sh.close()
        table.close()
        model.close()


# ------------------------------------------------------------ 2. loopback steps ----
LOOP = [(N, opt, kind, 16) for N in (1, 3) for opt in ("sgd", "momentum", "adagrad", "adam")
        for kind in ("deepfm", "lr")] + [(3, "adam", "deepfm", 8)]


@pytest.mark.parametrize("N,opt_kind,kind,k", LOOP, ids=["N%d-%s-%s-k%d" % c for c in LOOP])
def test_loopback_train_steps_equal_the_replicated_twin(N, opt_kind, kind, k):
    ctx, B = rmx.default_context(), 300
    ma, mb = make_model(kind, k, ctx), make_model(kind, k, ctx)
    n_mats = ma.matsLength()
    table = rmx.EmbeddingTable(ctx, V, k)
    table.fill_synthetic(SEED_TAB)
    sh = rmx.ShardedTable(ctx, V, k, N)
    sh.fill_synthetic(SEED_TAB)
    oa = rmx.Optimizer(ma, sh, opt_kind, **HYPER[opt_kind])
    ob = rmx.Optimizer(mb, table, opt_kind, **HYPER[opt_kind])
    try:
        for step in range(3):
            ids_h, tg_h = make_batch(200 + step, B)
            ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
            la = ma.train_step_sharded(sh, oa, B, ids, tg)
            lb = mb.train_step_ids(table, ob, B, ids, tg)
            what = "step %d" % (step + 1)
            assert np.float32(la) == np.float32(lb) and np.isfinite(la), what
            (sw, se), (tw, te) = shard_arrays(ctx, sh), table_arrays(ctx, table)
            assert np.array_equal(sw, tw) and np.array_equal(se, te), what
            assert np.array_equal(ma.getMats(), mb.getMats()), what
            assert np.float32(ma.getBias()) == np.float32(mb.getBias()), what
            st = shard_local_state(ctx, oa, k, sh.local_rows(), n_mats, N)
            tw_st = twin_state(ctx, ob, k, n_mats)
            assert_state_equal([s[0] for s in st], tw_st, rmx.OWNER_HASH_DEFAULT, N, k, what)
            for slot in range(2):
                for i, name in ((1, "mats"), (2, "bias")):
                    a, b = st[slot][i], tw_st[slot][i + 1]
                    assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (what, slot, name)
                assert (tw_st[slot][0] is not None) == (slot < NSLOTS[opt_kind])
            assert oa.steps == ob.steps == step + 1
            ids.free()
            tg.free()
        tw, te = table_arrays(ctx, table)
        w0 = rmx.EmbeddingTable(ctx, V, k)
        w0.fill_synthetic(SEED_TAB)
        assert not np.array_equal(table_arrays(ctx, w0)[0], tw)  # the steps did move the table
        w0.close()
    finally:
        oa.close()
        ob.close()
        sh.close()
        table.close()
        ma.close()
        mb.close()


# ------------------------------------------------------------ 3. / 4. groups ----
def _twin_reference(kind, k, opt_kind, steps, batches=None, grads=None, key=rmx.OWNER_HASH_DEFAULT):
    """The replicated twin: per step, per-rank backward_ids (or the given synthetic gradients), ids / g_w / g_emb
    concatenated in rank order, g_mats / g_bias added in rank order in np.float32, one apply with B = sum B_r.
    Returns per step (losses per rank, w, emb, mats, bias, state, steps)."""
    ctx = rmx.default_context()
    model = make_model(kind, k, ctx)
    n_mats = model.matsLength()
    table = rmx.EmbeddingTable(ctx, V, k)
    table.fill_synthetic(SEED_TAB)
    opt = rmx.Optimizer(model, table, opt_kind, **HYPER[opt_kind])
    out = []
    try:
        for step in range(steps):
            per = []
            if grads is not None:
                per = grads[step]
            else:
                for ids_h, tg_h in batches[step]:
                    B = len(tg_h)
                    ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
                    g = Grads(ctx, B * F, k, n_mats, kind == "lr")
                    model.backward_ids(table, B, ids, tg, *g.args())
                    d = g.numpy()
                    d["ids"] = ids_h
                    per.append(d)
                    for a in (g, ids, tg):
                        a.free()
            cat = lambda name: np.concatenate([d[name] for d in per])
            g_m, g_b = per[0]["g_mats"].copy(), per[0]["g_bias"].copy()
            for d in per[1:]:
                g_m = (g_m + d["g_mats"]).astype(np.float32)
                g_b = (g_b + d["g_bias"]).astype(np.float32)
            assert g_m.dtype == np.float32 and g_b.dtype == np.float32
            up = lambda a: rmx.DeviceArray.from_numpy(ctx, a)
            arrs = [up(cat("ids")), up(g_b), up(cat("g_w")), up(cat("g_emb")), up(g_m)]
            opt.apply(len(cat("ids")) // F, *arrs)
            ctx.sync()
            for a in arrs:
                a.free()
            w, e = table_arrays(ctx, table)
            out.append(dict(losses=[d.get("loss") for d in per], w=w, emb=e, mats=model.getMats(),
                            bias=np.float32(model.getBias()), state=twin_state(ctx, opt, k, n_mats),
                            steps=opt.steps))
    finally:
        opt.close()
        table.close()
        model.close()
    return out


def _check_group(res, ref, N, k, key, what):
    for step, want in enumerate(ref):
        for r in range(N):
            got = res[r][step]
            w = "%s step %d rank %d" % (what, step + 1, r)
            if want["losses"][r] is not None:
                assert np.float32(got["loss"]) == want["losses"][r][0], w
            assert np.array_equal(got["w"], want["w"]) and np.array_equal(got["emb"], want["emb"]), w
            assert np.array_equal(got["mats"], want["mats"]) and got["bias"] == want["bias"], w
            assert np.array_equal(got["mats"], res[0][step]["mats"]), w  # the replicas stay identical
            assert got["steps"] == want["steps"] == step + 1, w
            for slot in range(2):
                for i, name in ((1, "mats"), (2, "bias")):
                    a, b = got["state"][slot][i], want["state"][slot][i + 1]
                    assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (w, slot, name)
        parts = [[res[o][step]["state"][slot][0][0] for o in range(N)] for slot in range(2)]
        assert_state_equal(parts, want["state"], key, N, k, "%s step %d" % (what, step + 1))


GROUPS = [(2, "adam", "deepfm"), (2, "sgd", "deepfm"), (4, "adam", "deepfm"), (4, "sgd", "deepfm"),
          (2, "adam", "xdeepfm")]


@pytest.mark.parametrize("N,opt_kind,kind", GROUPS, ids=["N%d-%s-%s" % c for c in GROUPS])
def test_group_train_steps_equal_one_apply_on_the_concatenated_batches(N, opt_kind, kind):
    k, steps = 16, 2
    batches = [[make_batch(300 + 10 * step + r, BATCHES[r]) for r in range(N)] for step in range(steps)]
    ref = _twin_reference(kind, k, opt_kind, steps, batches=batches)
    g = rmx.ExchangeGroup(N)

    def rank(r):
        ctx = rmx.Context(0)
        sh = rmx.ShardedTable(ctx, V, k, N, r, group=g)
        sh.fill_synthetic(SEED_TAB)
        model = make_model(kind, k, ctx)
        n_mats = model.matsLength()
        opt = rmx.Optimizer(model, sh, opt_kind, **HYPER[opt_kind])
        out = []
        try:
            for step in range(steps):
                ids_h, tg_h = batches[step][r]
                ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
                loss = model.train_step_sharded(sh, opt, len(tg_h), ids, tg)
                w, e = shard_arrays(ctx, sh)
                out.append(dict(loss=loss, w=w, emb=e, mats=model.getMats(), bias=np.float32(model.getBias()),
                                state=shard_local_state(ctx, opt, k, sh.local_rows(), n_mats, 1),
                                steps=opt.steps))
                ids.free()
                tg.free()
        finally:
            opt.close()
            sh.close()
            model.close()
            ctx.close()
        return out

    try:
        res = _run_ranks(N, rank)
    finally:
        g.close()
    _check_group(res, ref, N, k, rmx.OWNER_HASH_DEFAULT, "%s %s" % (kind, opt_kind))


def _synthetic(seed, ids, k, n_mats):
    rng = np.random.default_rng(seed)
    n = len(ids)
    return dict(ids=ids, g_bias=rng.normal(0, 1, 1).astype(np.float32), g_w=rng.normal(0, 1, n).astype(np.float32),
                g_emb=rng.normal(0, 1, n * k).astype(np.float32), g_mats=rng.normal(0, 1, n_mats).astype(np.float32))


def _edge_ids(case):
    """Per-rank ids [300 * F] of the order edges, N = 3."""
    B, hot, per = 300, 1234, []
    for r in range(3):
        rng = np.random.default_rng(400 + r)
        ids = rng.integers(0, V, (B, F)).astype(np.int32)
        if case == "hot":
            # one id 600 times per rank: the list spans the ranks and its 512-chunks straddle their boundaries
            ids[:, 0] = ids[:, 1] = hot
            if r == 1:  # ids outside the table on one rank: skipped, never addressed
                ids[5, 2:9] = [V, V + 1, -1, -7, np.iinfo(np.int32).max, np.iinfo(np.int32).min, V + 77777]
        elif r == 2:  # owner = id mod 3 (key 0): everything this rank has goes to rank 0 -- empty buckets
            ids = (rng.integers(0, V // 3, (B, F)) * 3).astype(np.int32)
        per.append(ids.reshape(-1))
    return per


@pytest.mark.parametrize("case", ["hot", "empty-buckets"])
@pytest.mark.parametrize("opt_kind", ["adam", "sgd"])
def test_group_apply_order_edges(case, opt_kind):
    """rmx_optim_apply as a collective on synthetic gradients, N = 3: a hot id whose list spans the ranks, ids
    outside [0, V) on one rank, and (owner = id mod N) a rank whose ids all have one owner."""
    N, k, kind = 3, 16, "deepfm"
    key = 0 if case == "empty-buckets" else rmx.OWNER_HASH_DEFAULT
    probe = make_model(kind, k, None)
    n_mats = probe.matsLength()
    probe.close()
    ids = _edge_ids(case)
    if case == "hot":
        assert sum(int((i == 1234).sum()) for i in ids) >= 1800 and (ids[1] >= V).any() and (ids[1] < 0).any()
    else:
        assert (ids[2] % 3 == 0).all()
    grads = [[_synthetic(500 + 10 * step + r, ids[r], k, n_mats) for r in range(N)] for step in range(2)]
    ref = _twin_reference(kind, k, opt_kind, 2, grads=grads)
    g = rmx.ExchangeGroup(N)

    def rank(r):
        ctx = rmx.Context(0)
        sh = rmx.ShardedTable(ctx, V, k, N, r, group=g)
        sh.set_owner_hash(key)
        sh.fill_synthetic(SEED_TAB)
        model = make_model(kind, k, ctx)
        opt = rmx.Optimizer(model, sh, opt_kind, **HYPER[opt_kind])
        out = []
        try:
            for step in range(2):
                d = grads[step][r]
                arrs = [rmx.DeviceArray.from_numpy(ctx, d[n]) for n in ("ids", "g_bias", "g_w", "g_emb", "g_mats")]
                opt.apply(300, *arrs)
                ctx.sync()
                w, e = shard_arrays(ctx, sh)
                rec = dict(loss=None, w=w, emb=e, mats=model.getMats(), bias=np.float32(model.getBias()),
                           state=shard_local_state(ctx, opt, k, sh.local_rows(), n_mats, 1), steps=opt.steps)
                # an id outside the table still gathers zeros
                bad = rmx.DeviceArray.from_numpy(ctx, np.array([V, -1, V + 77777, 0], np.int32))
                bw, be = rmx.DeviceArray(ctx, 4, np.float32), rmx.DeviceArray(ctx, 4 * k, np.float32)
                sh.gather(bad, 4, bw, be)
                ctx.sync()
                rec["bad"] = (bw.numpy(), be.numpy())
                out.append(rec)
                for a in arrs + [bad, bw, be]:
                    a.free()
        finally:
            opt.close()
            sh.close()
            model.close()
            ctx.close()
        return out

    try:
        res = _run_ranks(N, rank)
    finally:
        g.close()
    _check_group(res, ref, N, k, key, "%s %s" % (case, opt_kind))
    for r in range(N):
        for rec in res[r]:
            bw, be = rec["bad"]
            assert not bw[:3].any() and not be[:3 * k].any() and bw[3] == rec["w"][0]


# ------------------------------------------------------------ 5. misuse ----
def _status(fn, *args):
    before = rmx.debug_live_device_memory()
    st = fn(*args)
    assert rmx.debug_live_device_memory() == before, "a refused call allocated or freed device memory"
    return st


def test_misuse_returns_its_code_and_touches_nothing():
    ctx, k, B = rmx.default_context(), 16, 64
    n = B * F
    L = _lib.lib
    model, model8 = make_model("deepfm", k, ctx), make_model("deepfm", 8, ctx)
    bf = rmx.DNN(V, F, k, FC, ctx=ctx)
    bf.setPrecision(rmx.DTYPE_BF16)
    bf.setMats(bf.initMats(SEED_MATS))
    bf.setBias(0.01)
    host_only = rmx.DeepFM(V, F, k, FC)
    table = rmx.EmbeddingTable(ctx, V, k)
    table.fill_synthetic(SEED_TAB)
    sh, sh2 = rmx.ShardedTable(ctx, V, k, 3), rmx.ShardedTable(ctx, V, k, 3)
    sh.fill_synthetic(SEED_TAB)
    sh2.fill_synthetic(SEED_TAB)
    o_sh = rmx.Optimizer(model, sh, "adam", eta=0.01)
    o_tab = rmx.Optimizer(model, table, "adam", eta=0.01)
    ids_h, tg_h = make_batch(7, B)
    ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
    g = Grads(ctx, n, k, model.matsLength(), False)
    gp = [a.ptr for a in g.args()]
    md, m8, mbf = model._device(), model8._device(), bf._device()
    loss = ctypes.c_float()
    try:
        bp = L.rmx_backward_pulled
        assert _status(bp, md, sh.handle, B, 0, tg.ptr, *gp, None) == _lib.RMX_E_INVALID  # empty slot
        sh.pull(ids, n, 0)
        assert _status(bp, md, sh.handle, B - 1, 0, tg.ptr, *gp, None) == _lib.RMX_E_SHAPE  # another id count
        assert _status(bp, mbf, sh.handle, B, 0, tg.ptr, *gp, None) == _lib.RMX_E_INVALID  # not fp32
        assert _status(bp, m8, sh.handle, B, 0, tg.ptr, *gp, None) == _lib.RMX_E_SHAPE  # k mismatch
        assert _status(bp, md, sh.handle, B, 2, tg.ptr, *gp, None) == _lib.RMX_E_INVALID  # no such slot
        assert _status(bp, md, None, B, 0, tg.ptr, *gp, None) == _lib.RMX_E_INVALID
        # slot 0 is busy: the step refuses it, and the pull in it survives every refused call above
        ts = L.rmx_train_step_sharded
        args = (B, ids.ptr, tg.ptr, ctypes.byref(loss), None)
        assert _status(ts, md, sh.handle, o_sh.handle, *args) == _lib.RMX_E_INVALID
        model.backward_pulled(sh, B, 0, tg, *g.args())
        ctx.sync()
        # the optimiser's argument checks, with the shard in the table's place
        h = ctypes.c_void_p()
        hy = (ctypes.c_double * 4)(0.01, 0.99, 0.9, 1e-7)
        cr = L.rmx_optim_create_sharded
        assert _status(cr, md, None, 3, hy, 4, ctypes.byref(h)) == _lib.RMX_E_INVALID
        assert _status(cr, None, sh.handle, 3, hy, 4, ctypes.byref(h)) == _lib.RMX_E_INVALID
        assert _status(cr, md, sh.handle, 3, hy, 4, None) == _lib.RMX_E_INVALID
        assert _status(cr, md, sh.handle, 4, hy, 1, ctypes.byref(h)) == _lib.RMX_E_INVALID  # unknown kind
        assert _status(cr, md, sh.handle, 0, hy, 2, ctypes.byref(h)) == _lib.RMX_E_INVALID  # SGD takes eta only
        assert _status(cr, md, sh.handle, 3, hy, 0, ctypes.byref(h)) == _lib.RMX_E_INVALID
        neg = (ctypes.c_double * 1)(-0.5)
        assert _status(cr, md, sh.handle, 0, neg, 1, ctypes.byref(h)) == _lib.RMX_E_INVALID
        nan = (ctypes.c_double * 1)(float("nan"))
        assert _status(cr, md, sh.handle, 0, nan, 1, ctypes.byref(h)) == _lib.RMX_E_INVALID
        assert _status(cr, host_only._meta, sh.handle, 3, hy, 4, ctypes.byref(h)) == _lib.RMX_E_INVALID
        assert _status(cr, mbf, sh.handle, 3, hy, 4, ctypes.byref(h)) == _lib.RMX_E_INVALID
        assert _status(cr, m8, sh.handle, 3, hy, 4, ctypes.byref(h)) == _lib.RMX_E_SHAPE
        assert not h.value
        # mixed use
        ti = L.rmx_train_step_ids
        assert _status(ti, md, table.handle, o_sh.handle, *args) == _lib.RMX_E_INVALID
        assert _status(ts, md, sh.handle, o_tab.handle, *args) == _lib.RMX_E_INVALID
        assert _status(ts, md, sh2.handle, o_sh.handle, *args) == _lib.RMX_E_INVALID
        assert _status(ts, m8, sh.handle, o_sh.handle, *args) == _lib.RMX_E_INVALID  # another model
        with pytest.raises(rmx.IllegalArgumentError):
            model.train_step_sharded(sh2, o_sh, B, ids, tg)
        with pytest.raises(rmx.IllegalArgumentError):
            model.train_step_ids(table, o_sh, B, ids, tg)
        sp = L.rmx_optim_shard_state_ptrs
        pw, pe = ctypes.c_void_p(), ctypes.c_void_p()
        assert _status(sp, o_tab.handle, 0, 0, ctypes.byref(pw), ctypes.byref(pe)) == _lib.RMX_E_INVALID
        assert _status(sp, o_sh.handle, 3, 0, ctypes.byref(pw), ctypes.byref(pe)) == _lib.RMX_E_INVALID
        assert _status(sp, o_sh.handle, 0, 2, ctypes.byref(pw), ctypes.byref(pe)) == _lib.RMX_E_INVALID
        assert o_sh.steps == 0 and o_tab.steps == 0
        # after all that, correct calls succeed
        assert np.isfinite(model.train_step_sharded(sh, o_sh, B, ids, tg))
        assert o_sh.steps == 1
    finally:
        for o in (o_sh, o_tab, g, ids, tg, sh, sh2, table, model, model8, bf, host_only):
            (o.free if isinstance(o, (Grads, rmx.DeviceArray)) else o.close)()


# ------------------------------------------------------------ 6. memory ----
def test_everything_closed_returns_the_device_memory():
    before = rmx.debug_live_device_memory()
    ctx, k = rmx.default_context(), 16
    for N in (1, 3):
        model = make_model("deepfm", k, ctx)
        sh = rmx.ShardedTable(ctx, V, k, N)
        sh.fill_synthetic(SEED_TAB)
        opt = rmx.Optimizer(model, sh, "adam", eta=0.01)
        for B in (64, 300):  # the second step grows every per-batch buffer
            ids_h, tg_h = make_batch(9, B)
            ids, tg = rmx.DeviceArray.from_numpy(ctx, ids_h), rmx.DeviceArray.from_numpy(ctx, tg_h)
            model.train_step_sharded(sh, opt, B, ids, tg)
            ids.free()
            tg.free()
        assert rmx.debug_live_device_memory()[0] > before[0]
        opt.close()
        sh.close()
        model.close()
        assert rmx.debug_live_device_memory() == before
    g = rmx.ExchangeGroup(2)

    def rank(r):
        c = rmx.Context(0)
        sh = rmx.ShardedTable(c, V, k, 2, r, group=g)
        sh.fill_synthetic(SEED_TAB)
        model = make_model("deepfm", k, c)
        opt = rmx.Optimizer(model, sh, "adam", eta=0.01)
        ids_h, tg_h = make_batch(10 + r, BATCHES[r])
        ids, tg = rmx.DeviceArray.from_numpy(c, ids_h), rmx.DeviceArray.from_numpy(c, tg_h)
        model.train_step_sharded(sh, opt, BATCHES[r], ids, tg)
        ids.free()
        tg.free()
        opt.close()
        sh.close()
        model.close()
        c.close()

    try:
        _run_ranks(2, rank)
    finally:
        g.close()
    assert rmx.debug_live_device_memory() == before
