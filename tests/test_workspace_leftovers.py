"""No kernel reads HBM scratch that its own call did not write (csrc/models.hip ensure_ws, the L-A staging,
csrc/train.hip ensure_train).

A model's workspaces only grow, are never cleared and are shared between forward and backward, so a kernel
that reads a pad column or a row past B sees what the previous, larger batch left there.  Every case primes
the model at a larger batch (the capacity then exceeds B and the leftovers are real data), fills the scratch
with zeros (rmx_debug_poison_workspace), runs and keeps the result, then for each pattern fills, runs again
and requires the result finite and BITWISE the kept one.  The patterns are bad values in both the fp32 and
the bf16 view of a word: a NaN (0x7FC07FC0), +Inf (0x7F800000, fp32 models only: as bf16 halves it is
[0, +Inf]) and ~1.0 (0x3F803F80: a ReLU turns a NaN into the 0 of a cleared buffer, only a plausible finite
value shows there).  The kept result is held to the oracle once per case at the project's bars (1e-5 fp32,
2e-4 against the bf16 emulation, test_train._close for gradients), and the stage list names the path the case
is about.  The backward cases also refill the five outputs with NaN before every call and poison LDS
(rmx_debug_fill_lds) with the same pattern."""
import numpy as np
import pytest

import rmx
import lifecycle_common as lc
from lifecycle_common import F, K
from test_train import _close

pytestmark = pytest.mark.gpu

NAN, INF, ONE = 0x7FC07FC0, 0x7F800000, 0x3F803F80
PRIME = 777


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    lc.restore_knobs()


def _patterns(bf16):
    return (NAN, ONE) if bf16 else (NAN, INF, ONE)


def _set(knobs):
    for k, v in knobs:
        rmx.set_tuning(k, v)


def _check_runs(m, run, patterns, lds_ctx=None):
    """run() -> list of fp32 arrays.  Fill 0 / run / keep, then each pattern: fill / run / compare."""
    def fill(pat):
        n = rmx.debug_poison_workspace(m, pat)
        assert n > 0, "the hook filled nothing"
        if lds_ctx is not None:
            rmx.debug_fill_lds(lds_ctx, pat)
        return n
    fill(0)
    m.set_timing(True)
    kept = run()
    stages = lc.stages_of(m)
    m.set_timing(False)
    for pat in patterns:
        fill(pat)
        got = run()
        for i, (g, k) in enumerate(zip(got, kept)):
            assert lc.same_bits(g, k), "pattern %s, output %d: %s" % (hex(pat), i, lc.diff_report(g, k))
    return kept, stages


def _forward_case(ctx, kind, B, bf16=False, knobs=(), expect=(), forbid=()):
    _set(knobs)
    m = lc.new_model(kind, bf16)
    t = lc.table(ctx, bf16)
    out = rmx.DeviceArray(ctx, PRIME, np.float32)
    m.forward_ids(t, PRIME, lc.dev_ids(ctx, PRIME, 11), out)  # prime: the capacity exceeds B
    ctx.sync()
    ids = lc.dev_ids(ctx, B)
    nan = np.full(PRIME, np.nan, np.float32)

    def run():
        out.upload(nan)
        m.forward_ids(t, B, ids, out)
        ctx.sync()
        full = out.numpy()
        assert np.isnan(full[B:]).all(), "the call wrote output rows past its batch"
        return [full[:B].copy()]

    (kept,), stages = _check_runs(m, run, _patterns(bf16))
    assert np.isfinite(kept).all()
    for s in expect:
        assert s in stages, (s, stages)
    for s in forbid:
        assert s not in stages, (s, stages)
    err = float(np.abs(kept - lc.oracle_forward(kind, B, 0, bf16)).max())
    print("%s B=%d bf16=%s: max |p - p_oracle| = %.3g, stages %s" % (kind, B, bf16, err, stages))
    assert err <= lc.forward_tol(bf16)


ENGINE = ("tower_layer1", "tower_layer2", "tower_layer3")
DEEPFM_PATHS = {
    "column_split": ((), ("encoder_fm_x",), ("tower_small", "tower_fused", "tower_tail")),
    "whole_tower": ((("s3_cols", 0),), ("tower_small",), ("encoder_fm_x",)),
    "fused": ((("s3_small", 0),), ("tower_fused",), ("encoder_fm_x", "tower_small")),
    "head_tail": ((("s3_small", 0), ("s3_fused", 0), ("s3_head", 2), ("s3_tail", 2)), ("tower_layer1", "tower_tail"),
                  ("tower_small", "tower_fused", "encoder_fm_x")),
    "engine": ((("s3_small", 0), ("s3_fused", 0), ("s3_head", 0), ("s3_tail", 0)), ENGINE,
               ("tower_small", "tower_fused", "tower_tail", "encoder_fm_x")),
}


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("path", list(DEEPFM_PATHS))
def test_deepfm_fp32_forward_paths(ctx, path, B):
    knobs, expect, forbid = DEEPFM_PATHS[path]
    _forward_case(ctx, "deepfm", B, knobs=knobs, expect=expect, forbid=forbid)


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("kind", ["dnn", "dcn", "pnn", "xdeepfm"])
def test_fp32_forward(ctx, kind, tail, B):
    """The per-layer engine at the defaults (these batches do not fill the chip), the row-owner tail forced."""
    extra = {"pnn": ("product",), "xdeepfm": ("cin_layer1", "cin_layer2", "cin_layer3+")}.get(kind, ())
    if tail:
        _forward_case(ctx, kind, B, knobs=(("s3_tail", 2),), expect=("tower_layer1", "tower_tail") + extra)
    else:
        _forward_case(ctx, kind, B, expect=ENGINE + extra, forbid=("tower_tail",))


@pytest.mark.parametrize("B", [37, 300])
def test_lr_forward(ctx, B):
    _forward_case(ctx, "lr", B, expect=("first_order_sigmoid",))


@pytest.mark.parametrize("B", [37, 300])
@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("kind", ["dcn", "pnn", "dnn", "deepfm"])
def test_bf16_forward(ctx, kind, tail, B):
    if tail:
        _forward_case(ctx, kind, B, bf16=True, knobs=(("bf16_tail", 1),), expect=("tower_layer1", "tower_tail"))
    else:
        _forward_case(ctx, kind, B, bf16=True, knobs=(("bf16_tail", 0),), expect=ENGINE, forbid=("tower_tail",))


# --- L-A: RecModel.forward on host arrays ------------------------------------------------------------------
LA_B = 37


def _la_case(kind, irregular, expect):
    B = LA_B
    m = lc.new_model(kind)
    lr = kind == "lr"
    mats = None if lr else lc.host_mats(kind)
    sizes = None if lr else m.getMatsSize()
    bias = np.array([lc.BIAS], np.float32)

    def fwd(b, row0, index):
        w, e = lc.host_rows(b, row0)
        batch = (index, lc.host_ids(b, row0).astype(np.int64))
        if lr:
            return m.forward(b, batch, bias, w)
        return m.forward(b, batch, bias, w, e, K, mats, sizes)

    index = lc.regular_index(B)
    if irregular:  # rows out of order: the first order goes through the CSR kernel into y12
        index = np.random.default_rng(1).permutation(index)
    prime_index = lc.regular_index(PRIME)
    fwd(PRIME, 11, np.random.default_rng(2).permutation(prime_index) if irregular else prime_index)
    (kept,), stages = _check_runs(m, lambda: [fwd(B, 0, index)], _patterns(False))
    assert np.isfinite(kept).all()
    for s in ("la_h2d",) + tuple(expect):
        assert s in stages, (s, stages)
    w, e = lc.host_rows(B, 0)
    import oracle_ctypes as oc
    ref = oc.forward(lc.orc_model(kind), B, index, bias, w, None if lr else e, mats, 1)
    err = float(np.abs(kept - ref).max())
    print("L-A %s irregular=%s: max |p - p_oracle| = %.3g, stages %s" % (kind, irregular, err, stages))
    assert err <= 1e-5


LA_STAGES = {"lr": ("first_order_sigmoid",), "deepfm": ("encoder_fm_x", "tower_layer3"), "dnn": ENGINE,
             "dcn": ENGINE, "pnn": ("product",) + ENGINE, "xdeepfm": ("cin_layer1",) + ENGINE}


@pytest.mark.parametrize("kind", lc.FP32_KINDS)
def test_la_forward_regular_index(kind):
    _la_case(kind, False, LA_STAGES[kind])


@pytest.mark.parametrize("kind", ["deepfm", "lr"])
def test_la_forward_irregular_index(kind):
    """The irregular index reaches y12 through the CSR first order (DeepFM then adds the FM to it: encoder_fm)."""
    _la_case(kind, True, ("encoder_fm",) if kind == "deepfm" else ("first_order_sigmoid",))


# --- backward ----------------------------------------------------------------------------------------------
def _backward_case(ctx, kind, B, prime, knobs=(), expect=()):
    _set(knobs)
    m = lc.new_model(kind)
    lc.Backward(ctx, kind, prime, lc.host_ids(prime, 11)).run(m)  # prime at the larger batch
    bw = lc.Backward(ctx, kind, B, lc.tie_free_ids(kind, B))
    kept, stages = _check_runs(m, lambda: bw.run(m), _patterns(False), lds_ctx=ctx)
    for name, g, wr in zip(lc.GRAD_NAMES, kept, lc.written(kind)):
        assert not wr or np.isfinite(g).all(), name
    for s in expect:
        assert s in stages, (s, stages)
    print("backward %s B=%d: stages %s" % (kind, B, stages))
    lc.assert_grads_match_oracle(kind, kept, lc.oracle_backward(kind, B), _close)


BACK_STAGES = {"lr": ("first_order_sigmoid",), "deepfm": ("encoder_fm_x", "tower_back1"),
               "dnn": ("gather_x", "tower_back1"), "dcn": ("cross", "cross_back", "tower_back1"),
               "pnn": ("product", "tower_back1"), "xdeepfm": ("cin_layer3+", "cin_back", "tower_back1")}


@pytest.mark.parametrize("kind", lc.FP32_KINDS)
def test_backward_default_paths(ctx, kind):
    _backward_case(ctx, kind, 300, PRIME, expect=BACK_STAGES[kind])


def test_backward_deepfm_head_x(ctx):
    """s3_head 2: the row-owner training head (head_x), its FM sums and ReLU bits in fms."""
    _backward_case(ctx, "deepfm", 4099, 5099, knobs=(("s3_head", 2),), expect=("head_x", "tower_back1"))


def test_backward_deepfm_row_owner_layers(ctx):
    """B = 20,000: the 400 x 400 hidden layers' forward and dX on the row-owner kernel (k_layer_s3.hip)."""
    _backward_case(ctx, "deepfm", 20_000, 21_000, expect=("head_x", "tower_layer2", "tower_back2"))


@pytest.mark.parametrize("kind", ["deepfm", "dcn"])
def test_backward_wgrad_sq_tile(ctx, kind):
    """B = 32,768 + 7: the 208 x 208 dW, its slice partial planes, the fused bias gradient, a ragged chunk."""
    _backward_case(ctx, kind, 32_775, 33_775, expect=("tower_layer2", "tower_back1", "tower_back2"))
