"""Device-resident optimiser step (rmx_optim_*, rmx_train_step_ids) on the GPU against tests/optim_ref.py.

V = 2,000 unless a test names its own (the radix-pass tables, the sweep's rows), so a batch holds many duplicate
ids.  The apply tests upload synthetic random gradients:
nothing there depends on the backward.

Bars.  Bitwise: SGD at eta = 1.0 (eta g is exact and p - g takes one rounding with or without an FMA), so the
fp32 reference in the contract's summation order must match bit for bit.  Numeric (Momentum, Adagrad, Adam):
|got - ref| <= 1e-5 max|ref| per array on parameter deltas and states against the fp64 formulas fed the
fp32-aggregated gradient -- an update is at most ~10 fp32 roundings ~ 6e-7 relative, and 1e-5 leaves headroom for
sqrt / div ulp differences; eta = 0.05 keeps a delta well above the ulp of the parameter it is read back from."""
import ctypes

import numpy as np
import pytest

import optim_ref as R
import rmx
from rmx import _lib

pytestmark = pytest.mark.gpu

V = 2000
FC = (24, 8)
NUM_BAR = 1e-5


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_model(kind, F, k, fc=FC, V=V):
    return {"lr": lambda: rmx.LR(V, F), "deepfm": lambda: rmx.DeepFM(V, F, k, list(fc)),
            "dnn": lambda: rmx.DNN(V, F, k, list(fc)), "dcn": lambda: rmx.DCN(V, F, k, 3, list(fc)),
            "pnn": lambda: rmx.PNN(V, F, k, list(fc)),
            "xdeepfm": lambda: rmx.XDeepFM(V, F, k, list(fc), [8, 4])}[kind]()


_TABLES = {}


def table_values(k, V=V):
    """The initial table of every test (computed once per k and V, never changed)."""
    if (k, V) not in _TABLES:
        rng = np.random.default_rng(1000 + k)
        if V <= 1 << 20:
            _TABLES[k, V] = (rng.uniform(-0.05, 0.05, V).astype(np.float32),
                             rng.uniform(-0.05, 0.05, (V, k)).astype(np.float32))
        else:  # a large table: drawn in fp32, and not kept
            return (rng.random(V, np.float32) * np.float32(0.1) - np.float32(0.05),
                    rng.random((V, k), np.float32) * np.float32(0.1) - np.float32(0.05))
    return _TABLES[k, V]


class Triple:
    """model + table + optimiser with known initial parameters."""

    def __init__(self, kind, F, k, opt_kind, fc=FC, bias=0.01, V=V, **hyper):
        self.ctx = rmx.default_context()
        self.kind, self.F, self.k, self.V = kind, F, k, V
        self.model = make_model(kind, F, k, fc, V)
        self.mats0 = self.model.initMats(0x3A75) if kind != "lr" else np.zeros(0, np.float32)
        if kind != "lr":
            self.model.setMats(self.mats0)
        self.model.setBias(bias)
        self.bias0 = np.float32(bias)
        self.w0, self.e0 = table_values(k, V)
        self.table = rmx.EmbeddingTable(self.ctx, V, k)
        self.table.upload(self.w0, self.e0)
        self.opt = rmx.Optimizer(self.model, self.table, opt_kind, **hyper)

    def read_table(self):
        pw, pe = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(_lib.lib.rmx_table_device_ptrs(self.table.handle, ctypes.byref(pw), ctypes.byref(pe)))
        self.ctx.sync()
        V = self.V
        w = rmx.DeviceArray(self.ctx, V, np.float32, pw, self.table).numpy()
        e = rmx.DeviceArray(self.ctx, V * self.k, np.float32, pe, self.table).numpy().reshape(V, self.k)
        return w, e

    def read_state(self, slot):
        p = [ctypes.c_void_p() for _ in range(4)]
        _lib.check(_lib.lib.rmx_optim_state_ptrs(self.opt.handle, slot, *[ctypes.byref(x) for x in p]))
        self.ctx.sync()
        sizes = (self.V, self.V * self.k, len(self.mats0), 1)
        return [rmx.DeviceArray(self.ctx, n, np.float32, x, self.opt).numpy() if x.value else None
                for x, n in zip(p, sizes)]

    def params(self):
        w, e = self.read_table()
        return dict(w=w, emb=e, mats=self.model.getMats(), bias=np.float32(self.model.getBias()))

    def ref(self, dtype):
        has_w, has_e = self.kind != "dnn", self.kind != "lr"
        kind = {v: n for n, v in rmx.Optimizer.KINDS.items()}[self.opt.kind]
        return R.RefOptim(kind, self.hp(), self.w0 if has_w else None, self.e0 if has_e else None,
                          self.mats0 if len(self.mats0) else None, self.bias0, dtype)

    def hp(self):
        return self._hp

    def close(self):
        self.opt.close()
        self.table.close()
        self.model.close()


def triple(kind, F, k, opt_kind, fc=FC, V=V, **hyper):
    t = Triple(kind, F, k, opt_kind, fc, V=V, **hyper)
    t._hp = R.hyper(opt_kind, **hyper)
    return t


def batch(seed, B, F, k, n_mats, hot=False, V=V):
    """ids [B * F] in [0, V) and synthetic per-nonzero gradients."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V, (B, F)).astype(np.int32)
    if hot:
        ids[:, 0] = min(1234, V - 1)  # one id B times: with B > 512 its list takes the chunk path
    nnz = B * F
    return dict(ids=ids.reshape(-1), g_bias=rng.normal(0, 1, 1).astype(np.float32),
                g_w=rng.normal(0, 1, nnz).astype(np.float32), g_emb=rng.normal(0, 1, (nnz, k)).astype(np.float32),
                g_mats=rng.normal(0, 1, n_mats).astype(np.float32))


def dev_apply(t, b, B):
    ctx = t.ctx
    up = lambda a: rmx.DeviceArray.from_numpy(ctx, a)
    arrs = dict(ids=up(b["ids"]), g_bias=up(b["g_bias"]), g_w=up(b["g_w"]), g_emb=up(b["g_emb"]),
                g_mats=up(b["g_mats"]) if len(b["g_mats"]) else None)
    t.opt.apply(B, arrs["ids"], arrs["g_bias"], arrs["g_w"], arrs["g_emb"], arrs["g_mats"])
    ctx.sync()
    for a in arrs.values():
        if a is not None:
            a.free()


def ref_apply(ref, b):
    ref.apply(b["ids"], b["g_bias"], b["g_w"], b["g_emb"], b["g_mats"] if len(b["g_mats"]) else None)


def assert_params_bitwise(t, ref, what=""):
    got = t.params()
    if ref.w is not None:
        assert same_bits(got["w"], ref.w), what + " w"
    else:
        assert same_bits(got["w"], t.w0), what + " w must be untouched"
    if ref.emb is not None:
        assert same_bits(got["emb"], ref.emb), what + " emb"
    else:
        assert same_bits(got["emb"], t.e0), what + " emb must be untouched"
    if ref.mats is not None:
        assert same_bits(got["mats"], ref.mats), what + " mats"
    assert same_bits(got["bias"], ref.bias), what + " bias"
    return got


# ------------------------------------------------------------------ apply, bitwise ----
BITWISE = [("deepfm", 37, 39, 16, False), ("deepfm", 512, 39, 16, False), ("deepfm", 600, 3, 16, True),
           ("deepfm", 37, 6, 4, False), ("lr", 37, 39, 16, False), ("dnn", 37, 39, 16, False),
           # tab_update_kernel<false> / tab_long_kernel<false> walk a row in 16-column chunks: one partial chunk
           # (k = 1, 5), two with a partial last one (k = 20), two full ones (k = 32); a hot id (> 512 occurrences)
           # takes tab_long_kernel<false> over two chunks (k = 20) and over a partial one (k = 5)
           ("deepfm", 37, 6, 1, False), ("deepfm", 37, 6, 5, False), ("deepfm", 37, 6, 20, False),
           ("deepfm", 37, 6, 32, False), ("deepfm", 600, 6, 20, True), ("deepfm", 600, 6, 5, True)]


@pytest.mark.parametrize("kind,B,F,k,hot", BITWISE, ids=["%s-B%d-F%d-k%d" % c[:4] for c in BITWISE])
def test_apply_sgd_bitwise(kind, B, F, k, hot):
    """One SGD apply at eta = 1.0: table w / emb, mats and bias equal the fp32 reference (sums in the contract
    order) bit for bit; rows whose id is not in the batch keep their bits; a group the model does not have (LR:
    embeddings, DNN: first order) is left alone."""
    t = triple(kind, F, k, "sgd", eta=1.0)
    try:
        b = batch(11 * B + F, B, F, k, len(t.mats0), hot)
        if hot:
            assert (b["ids"] == 1234).sum() > 512
        ref = t.ref(np.float32)
        ref_apply(ref, b)
        dev_apply(t, b, B)
        assert t.opt.steps == 1
        got = assert_params_bitwise(t, ref)
        untouched = np.ones(V, bool)
        untouched[b["ids"]] = False
        assert not untouched.all()
        assert untouched.any() or B * F > 5 * V  # (only the 512 x 39 nonzeros cover all 2,000 rows)
        assert same_bits(got["w"][untouched], t.w0[untouched])
        assert same_bits(got["emb"][untouched], t.e0[untouched])
        if kind != "dnn":
            assert np.all(got["w"][~untouched] != t.w0[~untouched])
    finally:
        t.close()


def test_apply_skips_ids_outside_the_table_and_null_groups():
    """Ids outside [0, V) contribute nothing and are never addressed; a NULL gradient leaves its group as it is."""
    B, F, k = 37, 6, 16
    t = triple("deepfm", F, k, "sgd", eta=1.0)
    try:
        b = batch(77, B, F, k, len(t.mats0))
        b["ids"][[0, 5, 17, 100]] = [-1, V, V + 12345, np.iinfo(np.int32).max]
        b["ids"][3] = np.iinfo(np.int32).min
        ref = t.ref(np.float32)
        ref.apply(b["ids"], None, b["g_w"], b["g_emb"], None)
        ids = rmx.DeviceArray.from_numpy(t.ctx, b["ids"])
        gw, ge = rmx.DeviceArray.from_numpy(t.ctx, b["g_w"]), rmx.DeviceArray.from_numpy(t.ctx, b["g_emb"])
        t.opt.apply(B, ids, None, gw, ge, None)
        t.ctx.sync()
        got = assert_params_bitwise(t, ref)
        assert same_bits(got["mats"], t.mats0) and got["bias"] == t.bias0
    finally:
        t.close()


RADIX_V = [(255, 1), (256, 2), (65535, 2), (65536, 3), (16_777_300, 4)]


@pytest.mark.parametrize("Vt,passes", RADIX_V, ids=["V%d" % v for v, _ in RADIX_V])
def test_apply_sgd_bitwise_radix_passes(Vt, passes):
    """The radix sort of the ids makes 1, 2, 3 or 4 passes (after an odd count of ping-pong passes the sorted keys
    lie in the other buffer): SGD at eta = 1.0 on a table of Vt rows, a few ids outside [0, Vt) -- Vt itself, the
    largest key, among them -- bit for bit against the reference."""
    assert R.radix_passes(Vt)[1] == passes
    B, F, k = 37, 6, 4
    t = triple("deepfm", F, k, "sgd", V=Vt, eta=1.0)
    try:
        b = batch(3 * passes + 1, B, F, k, len(t.mats0), V=Vt)
        b["ids"][[0, 5, 17, 100, 3]] = [-1, Vt, Vt + 12345, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
        b["ids"][[7, 8]] = [Vt - 1, 0]
        ref = t.ref(np.float32)
        ref_apply(ref, b)
        dev_apply(t, b, B)
        got = assert_params_bitwise(t, ref)
        inside = b["ids"][(b["ids"] >= 0) & (b["ids"] < Vt)]
        untouched = np.ones(Vt, bool)
        untouched[inside] = False
        assert same_bits(got["w"][untouched], t.w0[untouched])
        assert np.all(got["w"][~untouched] != t.w0[~untouched])
    finally:
        t.close()


def test_apply_sgd_bitwise_scan_scale():
    """nnz = 8,200 x 39 = 319,800 > 262,144: the histogram scan of a sort pass has more than one block of block
    sums to add."""
    B, F, k = 8200, 39, 16
    assert B * F > 262144
    t = triple("deepfm", F, k, "sgd", eta=1.0)
    try:
        b = batch(4242, B, F, k, len(t.mats0))
        ref = t.ref(np.float32)
        ref_apply(ref, b)
        dev_apply(t, b, B)
        assert_params_bitwise(t, ref)
    finally:
        t.close()


# ------------------------------------------------------------------ apply, numeric ----
@pytest.mark.parametrize("opt_kind,hyper", [("momentum", dict(eta=0.05)), ("adagrad", dict(eta=0.05)),
                                            ("adam", dict(eta=0.05))], ids=["momentum", "adagrad", "adam"])
def test_apply_numeric_three_steps(opt_kind, hyper):
    """Three consecutive applies with different batches: every step's parameter deltas and the states after it
    against the fp64 formulas (defaults for the other hyper-parameters) fed the fp32-aggregated gradient."""
    B, F, k = 64, 39, 16
    t = triple("deepfm", F, k, opt_kind, **hyper)
    try:
        ref = t.ref(np.float64)
        prev_got = dict(w=t.w0, emb=t.e0, mats=t.mats0, bias=t.bias0)
        worst = 0.0
        for step in range(3):
            b = batch(500 + step, B, F, k, len(t.mats0))
            prev_ref = dict(w=ref.w.copy(), emb=ref.emb.copy(), mats=ref.mats.copy(), bias=ref.bias.copy())
            ref_apply(ref, b)
            dev_apply(t, b, B)
            got = t.params()
            for name in ("w", "emb", "mats", "bias"):
                d_got = np.asarray(got[name], np.float64) - np.asarray(prev_got[name], np.float64)
                d_ref = getattr(ref, name) - prev_ref[name]
                err = np.abs(d_got.reshape(-1) - d_ref.reshape(-1)).max() / np.abs(d_ref).max()
                print("%s step %d delta %s: %.3g" % (opt_kind, step + 1, name, err))
                worst = max(worst, err)
                assert err <= NUM_BAR, (name, step, err)
            for slot in range(R.NSLOTS[opt_kind]):
                sw, se, sm, sb = t.read_state(slot)
                for name, g, r in (("w", sw, ref.s_w), ("emb", se, ref.s_emb), ("mats", sm, ref.s_mats),
                                   ("bias", sb, ref.s_bias)):
                    r = r[slot].reshape(-1)
                    err = np.abs(np.asarray(g, np.float64) - r).max() / np.abs(r).max()
                    print("%s step %d state %d %s: %.3g" % (opt_kind, step + 1, slot, name, err))
                    worst = max(worst, err)
                    assert err <= NUM_BAR, (name, slot, step, err)
            prev_got = got
        assert t.opt.steps == 3
        print("%s worst relative error %.3g" % (opt_kind, worst))
    finally:
        t.close()


@pytest.mark.parametrize("opt_kind", ["momentum", "adagrad", "adam"])
@pytest.mark.parametrize("kind", ["deepfm", "dnn"])
def test_apply_numeric_three_steps_k20(kind, opt_kind):
    """The same three steps at k = 20 -- two 16-column chunks per row, the second partial, in the stateful
    optimisers' update loops -- on DeepFM and on DNN (no first-order group: w and its states stay as they are)."""
    B, F, k = 64, 6, 20
    t = triple(kind, F, k, opt_kind, eta=0.05)
    try:
        ref = t.ref(np.float64)
        names = [n for n in ("w", "emb", "mats", "bias") if getattr(ref, n) is not None]
        assert ("w" in names) == (kind != "dnn") and "emb" in names
        prev_got = dict(w=t.w0, emb=t.e0, mats=t.mats0, bias=t.bias0)
        worst = 0.0
        for step in range(3):
            b = batch(700 + step, B, F, k, len(t.mats0))
            prev_ref = {n: np.array(getattr(ref, n), np.float64) for n in names}
            ref_apply(ref, b)
            dev_apply(t, b, B)
            got = t.params()
            for name in names:
                d_got = np.asarray(got[name], np.float64) - np.asarray(prev_got[name], np.float64)
                d_ref = np.asarray(getattr(ref, name), np.float64) - prev_ref[name]
                err = np.abs(d_got.reshape(-1) - d_ref.reshape(-1)).max() / np.abs(d_ref).max()
                worst = max(worst, err)
                assert err <= NUM_BAR, (name, step, err)
            if kind == "dnn":
                assert same_bits(got["w"], t.w0)
            for slot in range(R.NSLOTS[opt_kind]):
                sw, se, sm, sb = t.read_state(slot)
                for name, g, r in (("w", sw, ref.s_w), ("emb", se, ref.s_emb), ("mats", sm, ref.s_mats),
                                   ("bias", sb, ref.s_bias)):
                    if name not in names:
                        continue
                    r = np.asarray(r[slot], np.float64).reshape(-1)
                    err = np.abs(np.asarray(g, np.float64) - r).max() / np.abs(r).max()
                    worst = max(worst, err)
                    assert err <= NUM_BAR, (name, slot, step, err)
            prev_got = got
        assert t.opt.steps == 3
        print("%s %s k=20 worst relative error %.3g" % (kind, opt_kind, worst))
    finally:
        t.close()


# ------------------------------------------------------- repeatability and history ----
def test_apply_is_repeatable_across_fresh_triples():
    B, F, k = 512, 39, 16
    outs = []
    for _ in range(2):
        t = triple("deepfm", F, k, "adam", eta=0.05)
        try:
            dev_apply(t, batch(9, B, F, k, len(t.mats0)), B)
            p = t.params()
            outs.append([p["w"], p["emb"], p["mats"], p["bias"]] + [s for s in t.read_state(0)] +
                        [s for s in t.read_state(1)])
        finally:
            t.close()
    for a, b in zip(*outs):
        assert same_bits(a, b)


def test_apply_after_a_larger_batch_leaks_no_scratch():
    """B = 512, then B = 37 on the same optimiser: the second step equals, bit for bit, the reference continuing
    from the same state (the grouping scratch still holds the first step's 512 x 39 entries)."""
    F, k = 39, 16
    t = triple("deepfm", F, k, "sgd", eta=1.0)
    try:
        ref = t.ref(np.float32)
        for seed, B in ((21, 512), (22, 37)):
            b = batch(seed, B, F, k, len(t.mats0))
            ref_apply(ref, b)
            dev_apply(t, b, B)
            assert_params_bitwise(t, ref, "after B = %d:" % B)
        assert t.opt.steps == 2
    finally:
        t.close()


# ---------------------------------------------------------------- repack consistency ----
def _ids_targets(ctx, seed, B, F):
    rng = np.random.default_rng(seed)
    ids = rmx.DeviceArray.from_numpy(ctx, rng.integers(0, V, B * F).astype(np.int32))
    tg = rmx.DeviceArray.from_numpy(ctx, (rng.random(B) > 0.6).astype(np.float32))
    return ids, tg


@pytest.mark.parametrize("lines", [0, 1])
@pytest.mark.parametrize("kind", ["deepfm", "dcn", "pnn", "xdeepfm", "lr"])
def test_repack_consistency_after_train_steps(kind, lines):
    """After two train_step_ids the trained model's forward equals, bitwise, the forward of a fresh model given
    setMats(getMats()) / setBias(getBias()) and the same table: every packed form and host-side value was
    rebuilt from the updated mats, and (knob table_lines = 1) the table's line copy got the touched rows."""
    B, F, k = 37, 39, 16
    rmx.set_tuning("table_lines", lines)
    try:
        t = triple(kind, F, k, "adam", eta=0.01)
        try:
            ctx = t.ctx
            for step in range(2):
                ids, tg = _ids_targets(ctx, 40 + step, B, F)
                loss = t.model.train_step_ids(t.table, t.opt, B, ids, tg)
                assert np.isfinite(loss) and loss > 0
            assert t.opt.steps == 2
            mats, bias = t.model.getMats(), t.model.getBias()
            if kind != "lr":
                assert not same_bits(mats, t.mats0)
            assert bias != t.bias0
            out = rmx.DeviceArray(ctx, B, np.float32)
            t.model.forward_ids(t.table, B, ids, out)
            ctx.sync()
            trained = out.numpy()
            fresh = make_model(kind, F, k)
            try:
                if kind != "lr":
                    fresh.setMats(mats)
                fresh.setBias(bias)
                fresh.forward_ids(t.table, B, ids, out)
                ctx.sync()
                assert same_bits(trained, out.numpy())
                if lines:  # the line copy against the rows themselves: the same forward with the copy dropped
                    rmx.set_tuning("table_lines", 0)
                    t.table.refresh_lines()
                    fresh.forward_ids(t.table, B, ids, out)
                    ctx.sync()
                    assert same_bits(trained, out.numpy())
            finally:
                fresh.close()
        finally:
            t.close()
    finally:
        rmx.set_tuning("table_lines", None)


def _sweep_rows():
    import shape_cases as sc
    return [c.name for c in sc.CASES if not sc.backward_refused(c) and c.name != "lr_f1k16"]


@pytest.mark.parametrize("name", _sweep_rows())
def test_repack_consistency_sweep_rows(name):
    """The same off the tuned shape (shape_cases.py; LR once, no row whose backward is refused): after two
    train_step_ids at B = 37 the trained model's forward equals, bit for bit, that of a fresh model given getMats() /
    getBias() -- at B = 37 and at B = 16,400, where the large-batch tiles read other packed forms."""
    import shape_cases as sc
    c = sc.BY_NAME[name]
    ctx = rmx.default_context()
    rng = np.random.default_rng(90)
    Vs = sc.V
    m = sc.rmx_model(name)
    mats0, bias0 = m.getMats() if c.kind != "lr" else None, m.getBias()
    table = rmx.EmbeddingTable(ctx, Vs, c.k)
    table.upload(rng.uniform(-0.05, 0.05, Vs).astype(np.float32),
                 rng.uniform(-0.05, 0.05, (Vs, c.k)).astype(np.float32))
    opt = rmx.Optimizer(m, table, "adam", eta=0.01)
    fresh = None
    try:
        for step in range(2):
            ids = rmx.DeviceArray.from_numpy(ctx, rng.integers(0, Vs, 37 * c.F).astype(np.int32))
            tg = rmx.DeviceArray.from_numpy(ctx, (rng.random(37) > 0.6).astype(np.float32))
            loss = m.train_step_ids(table, opt, 37, ids, tg)
            assert np.isfinite(loss) and loss > 0
        mats, bias = (m.getMats() if c.kind != "lr" else None), m.getBias()
        assert bias != bias0 and (c.kind == "lr" or not same_bits(mats, mats0))
        fresh = sc.rmx_model(name)
        if c.kind != "lr":
            fresh.setMats(mats)
        fresh.setBias(bias)
        for B in (37, 16400):
            ids = rmx.DeviceArray.from_numpy(ctx, rng.integers(0, Vs, B * c.F).astype(np.int32))
            outs = []
            for mm in (m, fresh):
                out = rmx.DeviceArray(ctx, B, np.float32)
                mm.forward_ids(table, B, ids, out)
                ctx.sync()
                outs.append(out.numpy().copy())
            assert np.isfinite(outs[0]).all()
            assert same_bits(outs[0], outs[1]), (name, B, float(np.abs(outs[0] - outs[1]).max()))
    finally:
        if fresh is not None:
            fresh.close()
        opt.close()
        table.close()
        m.close()


# ---------------------------------------------------------- step = backward + apply ----
@pytest.mark.parametrize("kind", ["deepfm", "lr"])
def test_train_step_equals_backward_then_apply(kind):
    B, F, k = 64, 39, 16
    a = triple(kind, F, k, "adam", eta=0.05)
    b = triple(kind, F, k, "adam", eta=0.05)
    try:
        ctx = a.ctx
        ids, tg = _ids_targets(ctx, 61, B, F)
        loss_a = a.model.train_step_ids(a.table, a.opt, B, ids, tg)
        ml = max(len(b.mats0), 1)
        g_b, g_w = rmx.DeviceArray(ctx, 1, np.float32), rmx.DeviceArray(ctx, B * F, np.float32)
        g_e, g_m = rmx.DeviceArray(ctx, B * F * k, np.float32), rmx.DeviceArray(ctx, ml, np.float32)
        ls = rmx.DeviceArray(ctx, 1, np.float32)
        b.model.backward_ids(b.table, B, ids, tg, g_b, g_w, g_e if kind != "lr" else None,
                             g_m if kind != "lr" else None, ls)
        b.opt.apply(B, ids, g_b, g_w, g_e if kind != "lr" else None, g_m if kind != "lr" else None)
        ctx.sync()
        assert bits(np.float32(loss_a))[0] == bits(ls.numpy())[0]
        pa, pb = a.params(), b.params()
        for name in ("w", "emb", "mats", "bias"):
            assert same_bits(pa[name], pb[name]), name
        assert not same_bits(pa["w"], a.w0)
    finally:
        a.close()
        b.close()


# --------------------------------------------------------------------------- it learns ----
def test_it_learns():
    """DeepFM fc (16,), B = 256: labels = (first-order sum of a hidden random w* > 0); 30 Adam steps at eta = 0.01
    over the same batch bring the loss below 0.8 x the first step's."""
    B, F, k = 256, 39, 16
    t = triple("deepfm", F, k, "adam", fc=(16,), eta=0.01)
    try:
        rng = np.random.default_rng(2026)
        ids_h = rng.integers(0, V, (B, F)).astype(np.int32)
        w_star = rng.normal(0, 1, V)
        labels = (w_star[ids_h].sum(1) > 0).astype(np.float32)
        assert 0.3 < labels.mean() < 0.7
        ids = rmx.DeviceArray.from_numpy(t.ctx, ids_h.reshape(-1))
        tg = rmx.DeviceArray.from_numpy(t.ctx, labels)
        losses = [t.model.train_step_ids(t.table, t.opt, B, ids, tg) for _ in range(30)]
        print("losses: first %.4f last %.4f" % (losses[0], losses[-1]))
        assert losses[-1] < 0.8 * losses[0], losses
        assert t.opt.steps == 30
    finally:
        t.close()
