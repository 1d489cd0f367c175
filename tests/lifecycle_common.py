"""Shared pieces of test_workspace_leftovers.py and test_model_lifecycle.py: one shape (V = 20,000, F = 39,
k = 16, towers 400-400-400, CIN 200-200-200, cross depth 3), one synthetic table per dtype, and the oracle
references, each computed once and handed out read-only."""
import functools

import numpy as np

import oracle_ctypes as oc
import rmx

V, F, K = 20_000, 39, 16
FC, CIN, CROSS = (400, 400, 400), (200, 200, 200), 3
SEED_IDS, SEED_TAB, SEED_MATS = 0x5EED2026, 0x7AB1E, 0x3A75
BIAS = 0.01
FP32_KINDS = ["lr", "deepfm", "dnn", "dcn", "pnn", "xdeepfm"]
ORC = {"lr": oc.LR, "deepfm": oc.DEEPFM, "dnn": oc.DNN, "dcn": oc.DCN, "pnn": oc.PNN, "xdeepfm": oc.XDEEPFM}
# every knob a test of the two files may set: restored by their autouse fixtures
KNOBS = ("s3_cols", "s3_small", "s3_fused", "s3_head", "s3_tail", "bf16_tail")


def restore_knobs():
    for k in KNOBS:
        rmx.set_tuning(k, None)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def orc_model(kind):
    return oc.make_model(ORC[kind], F, K, fc=FC if kind != "lr" else (), cin=CIN if kind == "xdeepfm" else (),
                         cross_depth=CROSS if kind == "dcn" else 0)


@functools.lru_cache(None)
def host_mats(kind, bf16=False, seed=SEED_MATS):
    """initMats of the kind (orc_init_mats: the same bits as rmx_model_init_mats, test_abi.py); a bf16 model is
    given mats already rounded to bf16, as in test_bf16.py."""
    if kind == "lr":
        return _ro(np.zeros(0, np.float32))
    mats = oc.init_mats(orc_model(kind), seed)
    return _ro(oc.round_bf16(mats) if bf16 else mats)


def new_model(kind, bf16=False, mats=None):
    m = {"lr": lambda: rmx.LR(V, F), "deepfm": lambda: rmx.DeepFM(V, F, K, list(FC)),
         "dnn": lambda: rmx.DNN(V, F, K, list(FC)), "dcn": lambda: rmx.DCN(V, F, K, CROSS, list(FC)),
         "pnn": lambda: rmx.PNN(V, F, K, list(FC)),
         "xdeepfm": lambda: rmx.XDeepFM(V, F, K, list(FC), list(CIN))}[kind]()
    if bf16:
        m.setPrecision(rmx.DTYPE_BF16)
    if kind != "lr":
        m.setMats(host_mats(kind, bf16) if mats is None else mats)
    m.setBias(BIAS)
    return m


@functools.lru_cache(None)
def host_table(bf16=False):
    wt, et = oc.gen_table(SEED_TAB, V, K)
    if bf16:
        wt, et = oc.round_bf16(wt), oc.round_bf16(et)
    return _ro(wt), _ro(et)


_tables = {}


def table(ctx, bf16=False):
    if bf16 not in _tables:
        t = rmx.EmbeddingTable(ctx, V, K, rmx.DTYPE_BF16 if bf16 else rmx.DTYPE_F32)
        t.fill_synthetic(SEED_TAB)
        _tables[bf16] = t
    return _tables[bf16]


@functools.lru_cache(None)
def host_ids(B, row0=0):
    return _ro(oc.gen_ids(SEED_IDS, row0, B, F, V).astype(np.int32))


def dev_ids(ctx, B, row0=0):
    return rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(host_ids(B, row0)))


@functools.lru_cache(None)
def host_rows(B, row0=0, bf16=False):
    """(w, e): the table gather of host_ids(B, row0) -- what L-A callers pass as weights / embeddings."""
    wt, et = host_table(bf16)
    w, e = oc.gather(wt, et, 1, host_ids(B, row0).astype(np.int64))
    return _ro(w), _ro(e)


def regular_index(B):
    return np.repeat(np.arange(B, dtype=np.int64), F)


@functools.lru_cache(None)
def oracle_forward(kind, B, row0=0, bf16=False):
    """fp64 oracle (fp32 models) or the bf16 emulation on bf16-rounded parameters (bf16 models)."""
    w, e = host_rows(B, row0, bf16)
    lr = kind == "lr"
    return _ro(oc.forward(orc_model(kind), B, regular_index(B), np.array([BIAS], np.float32), w, None if lr else e,
                          None if lr else host_mats(kind, bf16), 2 if bf16 else 1))


def forward_tol(bf16):
    return 2e-4 if bf16 else 1e-5


def stages_of(m):
    names, _ = m.get_timing()
    return sorted(names)


def same_bits(a, b):
    """Bitwise equality of two fp32 arrays (NaNs included, -0 != +0)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff_report(got, kept):
    """How many entries differ, which come first, and the largest difference."""
    bad = np.flatnonzero(got.view(np.uint32) != kept.view(np.uint32))
    if bad.size == 0:
        return "identical"
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - kept.astype(np.float64))
    return "%d of %d entries differ (first %s, max |d| %.3g, %d not finite)" % (
        bad.size, got.size, bad[:8].tolist(), float(np.nanmax(d)) if np.isfinite(d).any() else float("nan"),
        int((~np.isfinite(got)).sum()))


# --- backward ---------------------------------------------------------------------------------------------
GRAD_NAMES = ("bias", "weights", "embedding", "mats", "loss")


def grad_sizes(kind, B):
    return (1, B * F, B * F * K, max(len(host_mats(kind)), 1), 1)


def written(kind):
    """Which of the five outputs rmx_backward_ids writes for the kind (the others keep the caller's bits)."""
    return (True, kind != "dnn", kind != "lr", kind != "lr", True)


@functools.lru_cache(None)
def host_targets(B):
    return _ro((np.random.default_rng(5).random(B) > 0.7).astype(np.float32))


class Backward:
    """One model's backward_ids calls on fixed ids / targets: the five outputs are filled with NaN by upload
    before every call, so a kernel that accumulates into an output it should overwrite shows up."""

    def __init__(self, ctx, kind, B, ids_host):
        self.ctx, self.kind, self.B = ctx, kind, B
        self.t = table(ctx)
        self.ids = rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(ids_host, np.int32).reshape(-1))
        self.targets = rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(host_targets(B)))
        self.outs = [rmx.DeviceArray(ctx, n, np.float32) for n in grad_sizes(kind, B)]
        self.nans = [np.full(n, np.nan, np.float32) for n in grad_sizes(kind, B)]

    def run(self, m):
        for o, n in zip(self.outs, self.nans):
            o.upload(n)
        g = self.outs
        m.backward_ids(self.t, self.B, self.ids, self.targets, g[0], g[1], g[2], g[3] if self.kind != "lr" else None,
                       g[4])
        self.ctx.sync()
        return [o.numpy().copy() for o in self.outs]


def backward_once(ctx, kind, B, row0=0, m=None):
    """One backward_ids of a (by default fresh) model on host_ids(B, row0)."""
    return Backward(ctx, kind, B, host_ids(B, row0)).run(m if m is not None else new_model(kind))


def assert_same_grads(got, kept, what):
    for name, a, b in zip(GRAD_NAMES, got, kept):
        assert same_bits(a, b), "%s: %s: %s" % (what, name, diff_report(a, b))


def _hidden_pre(kind, E, mats):
    """f64 pre-activations of every ReLU of the kind (tower layers, PNN layer 1, CIN maps), rows = samples."""
    B = E.shape[0]
    D = F * K
    mats = np.asarray(mats, np.float64)
    x = E.reshape(B, D)
    pres, off, fc = [], 0, FC
    if kind == "dcn":
        off = CROSS * D + CROSS
    if kind == "pnn":
        rows = [i for i in range(F) for j in range(i + 1, F)]
        cols = [j for i in range(F) for j in range(i + 1, F)]
        ip = (E[:, rows] * E[:, cols]).sum(2)
        P, D1 = len(rows), fc[0]
        pre = x @ mats[:D * D1].reshape(D1, D).T + ip @ mats[D * D1:(D + P) * D1].reshape(D1, P).T + mats[(D + P) * D1]
        pres.append(pre)
        x, off, fc = np.maximum(pre, 0), (D + P) * D1 + 1, fc[1:]
    for d in fc:
        K_ = x.shape[1]
        pre = x @ mats[off:off + K_ * d].reshape(d, K_).T + mats[off + K_ * d:off + K_ * d + d]
        pres.append(pre)
        x, off = np.maximum(pre, 0), off + K_ * d + d
    if kind == "xdeepfm":
        x0 = E.transpose(0, 2, 1).reshape(B * K, F)
        u, hp = x0, F
        for h in CIN:
            Z = (x0[:, :, None] * u[:, None, :]).reshape(B * K, F * hp)
            pre = Z @ mats[off:off + F * hp * h].reshape(h, F * hp).T + mats[off + F * hp * h:off + F * hp * h + h]
            pres.append(pre.reshape(B, K * h))
            u, off, hp = np.maximum(pre, 0), off + F * hp * h + h, h
    return pres


@functools.lru_cache(None)
def tie_free_ids(kind, B, row0=3, rel=1e-5):
    """B rows of ids whose ReLU inputs all stay clear of zero (test_train._tie_free: within fp32 rounding of 0
    the fp32 device and the f64 oracle may legitimately take different ReLU branches), picked from 2 B
    generated candidates."""
    cand = oc.gen_ids(SEED_IDS, row0, 2 * B, F, V).reshape(2 * B, F)
    if kind == "lr":
        return _ro(cand[:B].astype(np.int32))
    _, et = host_table()
    keep = []
    for c0 in range(0, 2 * B, 128 if kind == "xdeepfm" else 8192):
        E = et[cand[c0:c0 + (128 if kind == "xdeepfm" else 8192)].astype(np.int64)].astype(np.float64)
        ok = np.ones(E.shape[0], bool)
        for pre in _hidden_pre(kind, E, host_mats(kind)):
            ok &= (np.abs(pre) > rel * np.abs(pre).mean()).all(axis=1)
        keep.extend((c0 + np.flatnonzero(ok)).tolist())
        if len(keep) >= B:
            break
    assert len(keep) >= B, (kind, B, len(keep))
    return _ro(cand[keep[:B]].astype(np.int32))


@functools.lru_cache(None)
def oracle_backward(kind, B, row0=3):
    """The f64 oracle's gradients on tie_free_ids(kind, B, row0) and host_targets(B)."""
    ids = tie_free_ids(kind, B, row0).reshape(-1).astype(np.int64)
    wt, et = host_table()
    w, e = oc.gather(wt, et, 1, ids)
    return oc.backward(orc_model(kind), B, regular_index(B), np.array([BIAS], np.float32), w if kind != "dnn" else None,
                       e if kind != "lr" else None, host_mats(kind) if kind != "lr" else None, host_targets(B))


def assert_grads_match_oracle(kind, got, ref, close):
    """test_train's bars: the loss to 1e-5 relative, every gradient by test_train._close."""
    ml = len(host_mats(kind))
    assert abs(got[4][0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (got[4][0], ref["loss"])
    assert close(got[0], ref["bias"]), "bias"
    if kind != "dnn":
        assert close(got[1], ref["weights"]), "weights"
    if kind != "lr":
        assert close(got[2], ref["embedding"]), "embedding"
        assert close(got[3][:ml], ref["mats"]), "mats"
