"""One model object serves a whole run: its batch sizes go up and down, its mats are replaced, forward,
predict and backward are interleaved on it, and the same rows may arrive as host arrays (L-A) or as ids (L-B).

Every assertion here is BITWISE against a fresh model that was given the same call alone, and the stage lists
(set_timing / get_timing: which kernels ran) must be equal too -- a call's result and its kernel path depend on
this call's inputs, the knobs and the model, never on what the object was asked before.  (The fresh models'
results are held to the oracle by the other GPU test files at the same shapes; test_workspace_leftovers.py
anchors this shape.)"""
import numpy as np
import pytest

import rmx
import lifecycle_common as lc
from lifecycle_common import F, K

pytestmark = pytest.mark.gpu

MODELS = [(k, False) for k in lc.FP32_KINDS] + [("dcn", True), ("pnn", True)]
MODEL_IDS = ["%s%s" % (k, "_bf16" if b else "") for k, b in MODELS]
HISTORY = (300, 37, 2049, 1, 300, 2048, 777, 300)


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    lc.restore_knobs()


def _forward(ctx, m, B, bf16=False, row0=0):
    """(probabilities, stage list) of one forward_ids call."""
    out = rmx.DeviceArray(ctx, B, np.float32)
    out.upload(np.full(B, np.nan, np.float32))
    m.set_timing(True)
    m.forward_ids(lc.table(ctx, bf16), B, lc.dev_ids(ctx, B, row0), out)
    ctx.sync()
    stages = lc.stages_of(m)
    m.set_timing(False)
    return out.numpy().copy(), stages


def _backward(ctx, m, kind, B, row0=0):
    m.set_timing(True)
    g = lc.backward_once(ctx, kind, B, row0, m)
    stages = lc.stages_of(m)
    m.set_timing(False)
    return g, stages


_fresh = {}


def _fresh_forward(ctx, kind, bf16, B, mats_key=None, mats=None):
    """A fresh model's forward at B alone, computed once per (kind, dtype, B, mats, knobs in force)."""
    key = (kind, bf16, B, mats_key, tuple(rmx.get_tuning(k, -1) for k in lc.KNOBS))
    if key not in _fresh:
        _fresh[key] = _forward(ctx, lc.new_model(kind, bf16, mats), B, bf16)
    return _fresh[key]


def _assert_forward(got, ref, what):
    assert got[1] == ref[1], "%s: stages %s, a fresh model's %s" % (what, got[1], ref[1])
    assert lc.same_bits(got[0], ref[0]), "%s (stages %s): %s" % (what, got[1], lc.diff_report(got[0], ref[0]))


@pytest.mark.parametrize("kind,bf16", MODELS, ids=MODEL_IDS)
def test_batch_history_forward(ctx, kind, bf16):
    """Up and down, across the s3_cols boundary (2,048) and back: every call as from a fresh model."""
    m = lc.new_model(kind, bf16)
    for i, B in enumerate(HISTORY):
        _assert_forward(_forward(ctx, m, B, bf16), _fresh_forward(ctx, kind, bf16, B),
                        "%s call %d (B = %d) after %s" % (kind, i, B, list(HISTORY[:i])))


def test_batch_history_forward_deepfm_large(ctx):
    """DeepFM through the fused tower's batch (16,384) and back to the column-split path."""
    m = lc.new_model("deepfm")
    for i, B in enumerate((300, 16384, 300)):
        _assert_forward(_forward(ctx, m, B), _fresh_forward(ctx, "deepfm", False, B), "call %d (B = %d)" % (i, B))


def test_knob_history(ctx):
    """A DeepFM first called at B = 3,000 under the default s3_cols (2,048: not column-split), then at B = 3,000
    under s3_cols 4,096, against a fresh model under s3_cols 4,096."""
    m = lc.new_model("deepfm")
    first = _forward(ctx, m, 3000)
    assert "encoder_fm_x" not in first[1], first[1]
    rmx.set_tuning("s3_cols", 4096)
    ref = _fresh_forward(ctx, "deepfm", False, 3000)
    assert "encoder_fm_x" in ref[1], ref[1]
    _assert_forward(_forward(ctx, m, 3000), ref, "B = 3,000 under s3_cols 4,096 after B = 3,000 under the default")


@pytest.mark.parametrize("kind", lc.FP32_KINDS)
def test_batch_history_backward(ctx, kind):
    m = lc.new_model(kind)
    fresh = {}
    hist = (777, 300, 4099, 300)
    for i, B in enumerate(hist):
        if B not in fresh:
            fresh[B] = _backward(ctx, lc.new_model(kind), kind, B)
        got = _backward(ctx, m, kind, B)
        what = "%s backward call %d (B = %d) after %s" % (kind, i, B, list(hist[:i]))
        assert got[1] == fresh[B][1], "%s: stages %s, a fresh model's %s" % (what, got[1], fresh[B][1])
        lc.assert_same_grads(got[0], fresh[B][0], what)


@pytest.mark.parametrize("kind", ["deepfm", "dcn", "pnn", "xdeepfm"])
def test_interleaved_forward_backward_predict(ctx, kind):
    """forward_ids(300), backward_ids(512), forward_ids(300), predict_ids(1,000 rows by 300), forward_ids(300)."""
    n = 1000
    ids_n = lc.dev_ids(ctx, n, 21)

    def predict(mm):
        sc = rmx.DeviceArray(ctx, n, np.float32)
        sc.upload(np.full(n, np.nan, np.float32))
        mm.predict_ids(lc.table(ctx), n, ids_n, sc, batch=300)
        ctx.sync()
        return sc.numpy().copy()

    m = lc.new_model(kind)
    f1 = _forward(ctx, m, 300)
    b = _backward(ctx, m, kind, 512, 5)
    f2 = _forward(ctx, m, 300)
    p = predict(m)
    f3 = _forward(ctx, m, 300)
    ref = _fresh_forward(ctx, kind, False, 300)
    for i, f in enumerate((f1, f2, f3)):
        _assert_forward(f, ref, "%s forward %d of the interleaved run" % (kind, i + 1))
    bref = _backward(ctx, lc.new_model(kind), kind, 512, 5)
    assert b[1] == bref[1], (b[1], bref[1])
    lc.assert_same_grads(b[0], bref[0], "%s backward after a forward" % kind)
    pref = predict(lc.new_model(kind))
    assert lc.same_bits(p, pref), "predict after forward / backward: " + lc.diff_report(p, pref)


@pytest.mark.parametrize("kind,bf16", [("deepfm", False), ("xdeepfm", False), ("dcn", False), ("dcn", True)],
                         ids=["deepfm", "xdeepfm", "dcn", "dcn_bf16"])
def test_replaced_mats(ctx, kind, bf16):
    """setMats(A), forward, setMats(B), forward (+ backward): as from a fresh model that was given B only
    (xDeepFM packs its chunk-map planes at setMats, DCN recomputes its cross scalars there)."""
    mats_a = lc.host_mats(kind, bf16, 0xA11CE)
    mats_b = lc.host_mats(kind, bf16)
    assert not np.array_equal(mats_a, mats_b)
    m = lc.new_model(kind, bf16, mats_a)
    fa = _forward(ctx, m, 300, bf16)
    m.setMats(mats_b)
    fb = _forward(ctx, m, 300, bf16)
    ref = _fresh_forward(ctx, kind, bf16, 300)
    assert not lc.same_bits(fa[0], ref[0]), "the two mats give the same output: the case tests nothing"
    _assert_forward(fb, ref, "%s forward after setMats(A), forward, setMats(B)" % kind)
    if not bf16:  # (the backward is fp32 only)
        g = _backward(ctx, m, kind, 300, 5)
        gref = _backward(ctx, lc.new_model(kind), kind, 300, 5)
        assert g[1] == gref[1], (g[1], gref[1])
        lc.assert_same_grads(g[0], gref[0], "%s backward after replaced mats" % kind)


# --- L-A against L-B: the same rows as host arrays and as ids ------------------------------------------------
def _la_lb(ctx, kind, B, bf16=False):
    m = lc.new_model(kind, bf16)
    lb, _ = _forward(ctx, m, B, bf16)
    w, e = lc.host_rows(B, 0, bf16)  # the table gather of the same ids (a bf16 table's rows are exact in fp32)
    batch = (lc.regular_index(B), lc.host_ids(B).astype(np.int64))
    bias = np.array([lc.BIAS], np.float32)
    if kind == "lr":
        la = m.forward(B, batch, bias, w)
    else:
        la = m.forward(B, batch, bias, w, e, K, lc.host_mats(kind, bf16), m.getMatsSize())
    return la, lb


@pytest.mark.parametrize("B", [1, 100, 1024, 2048, 2049, 4096])
def test_la_equals_lb_deepfm_bitwise(ctx, B):
    """DeepFM fp32, one answer per input: rmx_forward on the gathered rows and rmx_forward_ids on their ids run
    the same kernels (B <= s3_cols: the column-split layers, layer 1 reading the staged rows in place and the
    encoder summing y1 + y2 in the order it does with ids; above it the whole-tower kernel for both)."""
    la, lb = _la_lb(ctx, "deepfm", B)
    assert lc.same_bits(la, lb), "B = %d: %s" % (B, lc.diff_report(la, lb))


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("kind,bf16", [("lr", False), ("dnn", False), ("dcn", False), ("pnn", False),
                                       ("xdeepfm", False), ("dcn", True), ("pnn", True), ("dnn", True),
                                       ("deepfm", True)],
                         ids=["lr", "dnn", "dcn", "pnn", "xdeepfm", "dcn_bf16", "pnn_bf16", "dnn_bf16", "deepfm_bf16"])
def test_la_close_to_lb(ctx, kind, bf16, B):
    """The other kinds: the two entries may sum in different orders (the first order by its own kernel or in
    layer 1's epilogue, say) -- within the cross-path bars of test_gpu_parity.py: 2e-6 fp32, 2e-4 bf16."""
    la, lb = _la_lb(ctx, kind, B, bf16)
    err = float(np.abs(la - lb).max())
    print("%s bf16=%s B=%d: max |L-A - L-B| = %.3g" % (kind, bf16, B, err))
    assert np.isfinite(la).all() and err <= (2e-4 if bf16 else 2e-6)
