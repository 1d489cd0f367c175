"""Dense random-weight parity of the fp32 towers and the CIN, measured where their output is visible.

With initMats weights the tower moves DeepFM's logit by a std of 0.010 against 0.185 for first order + FM, and
the 1e-5 bar on p cannot tell the 6-product split from a 2-term one (hi + mid only): 6e-8 in p.  Here the
output weights are multiplied by a power of two S (per model: CASES) so that the part of the logit the kernels
under test produce is at least half of the logit's std, and the comparison is on logit = log(p / (1 - p)) in
fp64, over the samples whose oracle p lies in [0.02, 0.98] (at most 2 % of a case may fall outside).

The bar comes from the reference alone.  On the same 512 rows
    e32 = max |logit(fp32 oracle) - logit(fp64 oracle)|      honest sequential fp32
    e2  = max |logit(2-term split) - logit(fp64 oracle)|     split_probes.forward_split(PRODUCTS_2TERM): every
                                                             tower / CIN / product Linear with weights and
                                                             activations cut to hi + mid
and a GPU path passes with max |logit(gpu) - logit(fp64 oracle)| <= e2 / 2: anything half as bad as losing the
lo parts fails.  test_reference_clearances (CPU) asserts e2 / 2 >= 2 e32 for every case, so honest fp32 has 2x
room, and that the oracle alone meets the exclusion cap and the visibility rule.  Measured: DESIGN.md §4
(split fp32 GEMM).
"""
import functools

import numpy as np
import pytest

import oracle_ctypes as oc
import rmx
import split_probes as sp

F, K, V = 39, 16, 50000
SEED_IDS, SEED_TAB, SEED_MATS = 0x5EED2026, 0x7AB1E, 0x3A75
BETA = 0.01
N_ROWS = 512
P_LO, P_HI, MAX_EXCLUDED = 0.02, 0.98, 0.02

# kind: oracle type, model shape, S, batches, initMats seed (SEED_MATS unless given)
CASES = {
    "deepfm": dict(t=oc.DEEPFM, kw=dict(fc=(400, 400, 400)), S=32, batches=(517, 2049, 9216)),
    "dnn": dict(t=oc.DNN, kw=dict(fc=(400, 400)), S=32, batches=(517, 2049)),
    "dcn": dict(t=oc.DCN, kw=dict(fc=(400, 400), cross_depth=3), S=32, batches=(517, 2049)),
    "pnn": dict(t=oc.PNN, kw=dict(fc=(400, 400)), S=32, batches=(517, 2049)),
    # (the pooled CIN maps are all positive: with most weight seeds their output dot is a constant of 1.5 - 3 in
    # the logit, whose fp32 partial sums alone cost e32 = 2 - 4e-6, more than e2 / 4; this seed centres the logit)
    "xdeepfm": dict(t=oc.XDEEPFM, kw=dict(fc=(400, 400), cin=(200, 200)), S=32, batches=(300, 4099),
                    seed=0x3FF45BD),
}


def _model(kind):
    kw = CASES[kind]["kw"]
    fc = list(kw["fc"])
    if kind == "deepfm":
        return rmx.DeepFM(V, F, K, fc)
    if kind == "dnn":
        return rmx.DNN(V, F, K, fc)
    if kind == "xdeepfm":
        return rmx.XDeepFM(V, F, K, fc, list(kw["cin"]))
    if kind == "dcn":
        return rmx.DCN(V, F, K, kw["cross_depth"], fc)
    return rmx.PNN(V, F, K, fc)


def _out_slice(kind, n):
    """Where in mats the output weights fed by the kernels under test lie: the tower's 400 (DeepFM, DNN, PNN:
    before b_out; DCN: after the cross part of its bias-free output Linear), xDeepFM: CIN pools + tower."""
    if kind in ("deepfm", "dnn", "pnn"):
        return slice(n - 401, n - 1)
    if kind == "dcn":
        return slice(n - 400, n)
    return slice(n - (sum(CASES[kind]["kw"]["cin"]) + 400), n)


@functools.lru_cache(maxsize=None)
def scaled_mats(kind):
    om = oc.make_model(CASES[kind]["t"], F, K, **CASES[kind]["kw"])
    mats = oc.init_mats(om, CASES[kind].get("seed", SEED_MATS))
    mats[_out_slice(kind, mats.size)] *= np.float32(CASES[kind]["S"])
    mats.setflags(write=False)
    return mats


def oracle_rows(B):
    """512 rows of a batch: head, middle and tail thirds (all rows of a smaller batch)."""
    if B <= N_ROWS:
        return np.arange(B)
    a = N_ROWS // 3
    return np.concatenate([np.arange(a + N_ROWS - 3 * a), B // 2 - a // 2 + np.arange(a), B - a + np.arange(a)])


def logit(p):
    p = np.asarray(p, np.float32).astype(np.float64)
    return np.log(p / (1.0 - p))


@functools.lru_cache(maxsize=None)
def inputs(kind, B):
    """(oracle model, rows, n, index, bias, gathered weights, gathered embeddings) of a case's oracle rows."""
    c = CASES[kind]
    rows = oracle_rows(B)
    n = rows.size
    wt, et = oc.gen_table(SEED_TAB, V, K)
    ids = oc.gen_ids(SEED_IDS, 0, B, F, V).reshape(B, F)[rows].astype(np.int64).ravel()
    w, e = oc.gather(wt, et, 1, ids)
    return (oc.make_model(c["t"], F, K, **c["kw"]), rows, n, np.repeat(np.arange(n, dtype=np.int64), F),
            np.array([BETA], np.float32), w, e)


def emulate(keep, kind, B):
    """p (fp32, as a kernel stores it) of the split emulation keeping the products `keep`, on the oracle rows."""
    om, rows, n, index, bias, w, e = inputs(kind, B)
    return sp.forward_split(keep, kind, n, F, K, index, bias, w, e, scaled_mats(kind),
                            **CASES[kind]["kw"]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(kind, B):
    """The references on the case's oracle rows, computed once and shared (read-only)."""
    om, rows, n, index, bias, w, e = inputs(kind, B)
    mats = scaled_mats(kind)
    p64 = oc.forward(om, n, index, bias, w, e, mats, 1)
    p32 = oc.forward(om, n, index, bias, w, e, mats, 0)
    p2 = emulate(sp.PRODUCTS_2TERM, kind, B)
    keep = (p64 >= P_LO) & (p64 <= P_HI)
    l64 = logit(p64)
    res = dict(rows=rows, keep=keep, l64=l64, e32=float(np.abs(logit(p32) - l64)[keep].max()),
               e2=float(np.abs(logit(p2) - l64)[keep].max()))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def kernels_part(kind, B):
    """The part of the fp64 oracle's logit that the kernels' output weights carry: the logit minus the one with
    those weights zeroed (what is left is first order, FM / cross, biases)."""
    om, rows, n, index, bias, w, e = inputs(kind, B)
    m0 = np.array(scaled_mats(kind))
    m0[_out_slice(kind, m0.size)] = 0
    return reference(kind, B)["l64"] - logit(oc.forward(om, n, index, bias, w, e, m0, 1))


ALL_CASES = [(kind, B) for kind, c in CASES.items() for B in c["batches"]]


@pytest.mark.parametrize("kind,B", ALL_CASES)
def test_reference_clearances(kind, B):
    """Against the oracle alone: the bar e2 / 2 leaves honest sequential fp32 2x room, the exact 6-product
    split emulation passes it, at most 2 % of the rows are excluded, nothing saturates, and the kernels' part is
    at least half of the logit's std."""
    r = reference(kind, B)
    part = kernels_part(kind, B)
    e6 = float(np.abs(logit(emulate(sp.PRODUCTS6, kind, B)) - r["l64"])[r["keep"]].max())
    print("%s B=%d: e32 %.3g, 6-product emulation %.3g, e2 %.3g (bar %.3g); excluded %d of %d; std part %.3g of "
          "logit %.3g; |logit| <= %.3g" % (kind, B, r["e32"], e6, r["e2"], r["e2"] / 2, (~r["keep"]).sum(),
                                          r["keep"].size, part.std(), r["l64"].std(), np.abs(r["l64"]).max()))
    assert r["e2"] / 2 >= 2 * r["e32"]
    assert e6 <= r["e2"] / 2
    assert (~r["keep"]).mean() <= MAX_EXCLUDED
    assert np.isfinite(r["l64"]).all()
    assert part.std() >= 0.5 * r["l64"].std()


@pytest.mark.parametrize("kind", ["deepfm", "dnn", "dcn", "pnn"])
def test_bar_catches_a_dropped_product(kind):
    """The power of the bar, on the CPU: the emulation with one product left out of every layer.  Without hi x hi,
    hi x mid or mid x hi it is over the bar by more than 100x.  One of the three smallest products alone (hi x lo,
    lo x hi, mid x mid) is half of what the bar is built from (e2 drops two), so it lands at about 1 - 2x the bar
    (DNN without lo x hi: 7.18e-6 on a bar of 7.18e-6): printed, not asserted -- the exact probes
    (test_split_probes.py) are the test for a single small product."""
    B = CASES[kind]["batches"][0]
    r = reference(kind, B)
    for gone in sp.PRODUCTS6:
        p = emulate(tuple(q for q in sp.PRODUCTS6 if q != gone), kind, B)
        err = float(np.abs(logit(p) - r["l64"])[r["keep"]].max())
        print("%s B=%d without %s: %.3g (bar %.3g)" % (kind, B, gone, err, r["e2"] / 2))
        if gone in ("hh", "hm", "mh"):
            assert err > 100 * r["e2"] / 2, gone
    assert r["e2"] > r["e2"] / 2 > 0  # (the 2-term split itself: over the bar by construction)


# ---------------------------------------------------------------- GPU -------
KNOBS = ("s3_small", "s3_fused", "s3_head", "s3_tail", "s3_cols", "f32_split", "cin_narrow", "s3_cin")

# DeepFM paths as in test_split_probes.py (cols: the knob lifts its batch limit for B = 2,049)
DEEPFM_PATHS = {
    "cols": ({"s3_cols": 1 << 20}, "encoder_fm_x"),
    "small": ({"s3_small": 2}, "tower_small"),
    "fused": ({"s3_fused": 2, "s3_small": 0}, "tower_fused"),
    "head_tail": ({"s3_fused": 0, "s3_head": 2, "s3_tail": 2, "s3_small": 0}, "tower_tail"),
    "generic": ({"s3_fused": 0, "s3_head": 0, "s3_tail": 0, "s3_small": 0}, "tower_layer3"),
    "f32_mfma": ({"f32_split": 0}, "tower_layer3"),
}


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    for k in KNOBS:
        rmx.set_tuning(k, None)


class _Case:
    """A model with the scaled mats, the synthetic table and ids of one (kind, B) on the device."""

    def __init__(self, ctx, kind, B):
        self.ctx, self.kind, self.B = ctx, kind, B
        self.m = _model(kind)
        self.m.setMats(scaled_mats(kind))
        self.m.setBias(BETA)
        self.table = rmx.EmbeddingTable(ctx, V, K)
        self.table.fill_synthetic(SEED_TAB)
        self.ids = rmx.DeviceArray(ctx, B * F, np.int32)
        rmx.gen_ids(ctx, SEED_IDS, 0, B, F, V, self.ids)
        self.out = rmx.DeviceArray(ctx, B, np.float32)
        self.ref = reference(kind, B)

    def run(self, knobs, stage=None):
        for k in KNOBS:
            rmx.set_tuning(k, None)
        for k, v in knobs.items():
            rmx.set_tuning(k, v)
        m = self.m
        m.set_timing(True)
        m.forward_ids(self.table, self.B, self.ids, self.out)
        self.ctx.sync()
        stages, _ = m.get_timing()
        m.set_timing(False)
        if stage:
            assert stage in stages, (knobs, list(stages))
        r = self.ref
        p = self.out.numpy()[r["rows"]]
        assert np.isfinite(p).all()
        err = np.abs(logit(p) - r["l64"])[r["keep"]]
        e = float(err.max())
        print("%s B=%d %s: max|logit - logit_fp64| = %.3g  (e32 %.3g, e2 %.3g, bar %.3g)" % (
            self.kind, self.B, knobs, e, r["e32"], r["e2"], r["e2"] / 2))
        assert e <= r["e2"] / 2, (self.kind, self.B, knobs, list(stages))
        return e


@pytest.mark.gpu
@pytest.mark.parametrize("B", CASES["deepfm"]["batches"])
def test_deepfm_logit_parity_on_every_path(ctx, B):
    c = _Case(ctx, "deepfm", B)
    for path, (knobs, stage) in DEEPFM_PATHS.items():
        if B == 9216 and path != "fused":
            continue  # (the batch the fused tower takes by default)
        c.run(knobs, stage)
    if B == 9216:
        c.run({}, "tower_fused")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [(k, B) for k in ("dnn", "dcn", "pnn") for B in CASES[k]["batches"]])
def test_tower_models_logit_parity(ctx, kind, B):
    c = _Case(ctx, kind, B)
    c.run({}, "tower_layer2")
    c.run({"f32_split": 0}, "tower_layer2")


@pytest.mark.gpu
@pytest.mark.parametrize("B", CASES["xdeepfm"]["batches"])
def test_xdeepfm_logit_parity_cin_variants(ctx, B):
    c = _Case(ctx, "xdeepfm", B)
    for narrow in (1, 0):
        for var in range(5):
            c.run({"cin_narrow": narrow, "s3_cin": var}, "cin_layer2")
    c.run({"f32_split": 0}, "cin_layer2")
