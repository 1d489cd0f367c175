"""Every model off the benchmark shape at the batches that pick kernels (shape_cases.py, "the batch axis"): the
forward of every row on FWD_LADDER / CIN_LADDER in fp32 and on BF16_LADDER in bf16, the backward of the (row, batch)
list BWD_RUNS, against the oracle at the project's bars -- |p - p64| <= 1e-5, <= 2e-4 against the bf16 emulation,
test_train's bars for the loss and the gradients.  Ids come from rmx.gen_ids on the device; the forward's oracle
runs on three slices of the batch (its head, its last rows and rows straddling a 256-row block boundary in the
middle), the backward's on the whole batch.  test_shape_sweep_cpu.py holds what makes a failure here the kernels':
every batch-selected kernel is claimed by a (row, batch) run here (test_ladder_reaches_every_path), and leaving
the last partial 32-row chunk out of the batch sums breaks the gradient bars (test_tail_sensitivity)."""
import functools

import numpy as np
import pytest

import oracle_ctypes as oc
import rmx
import shape_cases as sc
from grad_check import _close
from rmx import _lib
from shape_cases import BY_NAME, TOL, TOL_BF16, V
from test_shape_sweep import NAN, ONE, _Backward, _forward_ids, _same_bits, _stages

pytestmark = pytest.mark.gpu

BF16_RUN = [n for n in sc.BF16_NAMES if not sc.bf16_refused(BY_NAME[n])]
LAYER_STAGES = ("tower_layer1", "tower_layer2", "tower_layer3", "tower_layer4+")
HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63  # hip_runtime_api.h hipDeviceAttribute_t (ROCm 6 / 7)


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(scope="module")
def ncu(ctx):
    """The device's CU count: the split GEMM, the CIN and the 208 x 208 dW choose by it."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    dev, n = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.hipGetDevice(ctypes.byref(dev)) == 0
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, dev) == 0
    print("CU count %d" % n.value)
    assert 0 < n.value <= 4096
    return n.value


def slices(B):
    """(first row, rows) of the oracle's slices of a batch of B."""
    if B <= 1200:
        return ((0, B),)
    mid = B // 2 // 256 * 256
    return ((0, 512), (mid - 150, 300), (B - 300, 300))


@functools.lru_cache(None)
def reference(name, B, bf16=False):
    """[(first row, oracle probabilities)]: f64, or the bf16 emulation on bf16-rounded parameters."""
    c = BY_NAME[name]
    return tuple((r0, sc._ro(sc.oracle_on(c, oc.gen_ids(sc.SEED_IDS, r0, n, c.F, V), 2 if bf16 else 1, bf16)))
                 for r0, n in slices(B))


def dev_ids(ctx, c, B):
    ids_d = rmx.DeviceArray(ctx, B * c.F, np.int32)
    rmx.gen_ids(ctx, sc.SEED_IDS, 0, B, c.F, V, ids_d)
    return ids_d


def worst_error(name, B, got, bf16=False):
    return max(float(np.abs(got[r0:r0 + len(ref)] - ref).max()) for r0, ref in reference(name, B, bf16))


def tiles_text(c, B, ncu, bf16=False):
    t = ["L%d %s/%s" % (i + 1, e, t) for i, e, t in sc.fwd_tiles(c, B, ncu, bf16)]
    return ", ".join(t + ["cin%d %s" % (i + 1, t) for i, t in sc.cin_tiles(c, B, ncu)]) or "-"


def check_claims(name, B, ncu, preds):
    """What shape_cases.CLAIMS says of (name, B) among `preds` holds on this device's CU count too: on a part
    where it does not, the claimed kernel is not the one that ran, and the run fails rather than pass unseen."""
    for r, b, p in sc.claims_of(preds):
        if (r, b) == (name, B):
            assert preds[p](BY_NAME[name], B, ncu), "%s at B = %d does not reach %s on %d CUs" % (name, B, p, ncu)


# ---- forward, fp32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_forward_ladder_fp32(ctx, ncu, name):
    c = BY_NAME[name]
    m = sc.rmx_model(name)
    t = sc.dev_table(ctx, c.k)
    for B in sc.ladder(c):
        ids_d = dev_ids(ctx, c, B)
        m.set_timing(True)
        got = _forward_ids(ctx, m, t, B, ids_d)
        stages = _stages(m)
        m.set_timing(False)
        err = worst_error(name, B, got)
        print("%s B=%d: max |p - p64| = %.3g; %s; stages %s" % (name, B, err, tiles_text(c, B, ncu), sorted(stages)))
        assert got.shape == (B,) and np.isfinite(got).all()
        assert err <= TOL, (name, B, err)
        check_claims(name, B, ncu, sc.FWD_PRED)
        again = _forward_ids(ctx, m, t, B, ids_d)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), (name, B, "a second launch differs")
        # the path is the point: DeepFM leaves the column-split path above s3_cols, and with k = 16 and a
        # split-GEMM layer 1 the first order and the FM ride that layer -- at F = 13, 26 and 39 alike
        if sc.encoder_fm_x(c):
            assert "encoder_fm_x" not in stages, (name, B, sorted(stages))
        if sc.deepfm_fm_fused_layer1(c, B):
            assert stages == set(LAYER_STAGES[:len(c.fc)]), (name, B, sorted(stages))
        elif c.kind == "deepfm" and c.fc[0] != 400:
            assert "encoder_fm" in stages, (name, B, sorted(stages))
        if c.kind == "xdeepfm":
            assert "cin_layer1" in stages
        ids_d.free()
    m.close()


# ---- forward, bf16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BF16_RUN)
def test_forward_ladder_bf16(ctx, ncu, name):
    c = BY_NAME[name]
    m = sc.rmx_model(name, bf16=True)
    t = sc.dev_table(ctx, c.k, bf16=True)
    for B in sc.BF16_LADDER:
        ids_d = dev_ids(ctx, c, B)
        got = _forward_ids(ctx, m, t, B, ids_d)
        err = worst_error(name, B, got, True)
        print("%s B=%d bf16: max |p - p_bf16 oracle| = %.3g; %s" % (name, B, err, tiles_text(c, B, ncu, True)))
        assert got.shape == (B,) and np.isfinite(got).all()
        assert err <= TOL_BF16, (name, B, err)
        check_claims(name, B, ncu, sc.BF16_PRED)
        ids_d.free()
    m.close()


# ---- forward leftovers: the K tails of the large-batch split tiles ---------------------------------------
K_TAIL_RUNS = sorted({(r, B) for r, B, _ in sc.claims_of(("s3_dense16_K_tail", "s3_wave8_K_tail"))})


@pytest.mark.parametrize("name,B", K_TAIL_RUNS)
def test_forward_leftovers(ctx, name, B):
    """The 16-byte slot that runs past K = 413 or 37 on the 8-wave and 16-wave tiles: primed at 65,573, so that the
    workspace is larger than the call's, then the scratch and every CU's LDS hold NaNs or ones before the call."""
    c = BY_NAME[name]
    m = sc.rmx_model(name)
    t = sc.dev_table(ctx, c.k)
    big = sc.FWD_LADDER[-1]
    prime = dev_ids(ctx, c, big)
    _forward_ids(ctx, m, t, big, prime)
    prime.free()
    ids_d = dev_ids(ctx, c, B)
    kept = None
    for pat in (0, NAN, ONE):
        assert rmx.debug_poison_workspace(m, pat) > 0
        rmx.debug_fill_lds(ctx, pat)
        got = _forward_ids(ctx, m, t, B, ids_d)
        if kept is None:
            kept = got
            assert np.isfinite(kept).all() and worst_error(name, B, kept) <= TOL
        assert _same_bits(got, kept), "%s B=%d, pattern %s: max |d| %s" % (name, B, hex(pat), np.abs(got - kept).max())
    ids_d.free()
    m.close()


# ---- backward --------------------------------------------------------------------------------------------
def backward_at(ctx, name, B):
    c = BY_NAME[name]
    return _Backward(ctx, c, B, sc.tie_free_ids(name, B))


def check_backward_stages(c, stages):
    def want(stage, on):
        assert (stage in stages) == bool(on), "%s: stage %s %s: %s" % (c.name, stage, "missing" if on else
                                                                         "not expected", sorted(stages))
    fused = sc.head_fused(c)
    want("head_bce", fused)
    for s in ("tower_head", "bce", "head_back"):
        want(s, not fused)
    want("emb_grad", not sc.emb_fused(c))
    want("cin_back", c.kind == "xdeepfm")
    want("cross_back", c.kind == "dcn")


@pytest.mark.parametrize("name,B", sc.BWD_RUNS)
def test_backward_ladder(ctx, ncu, name, B):
    c = BY_NAME[name]
    m = sc.rmx_model(name)
    bw = backward_at(ctx, name, B)
    m.set_timing(True)
    g_b, g_w, g_e, g_m, loss = bw.run(m)
    stages = _stages(m)
    m.set_timing(False)
    ref = sc.oracle_backward(name, B)
    pairs = [("bias", g_b, ref["bias"])] + ([("weights", g_w, ref["weights"])] if c.kind != "dnn" else []) + \
        [("embedding", g_e, ref["embedding"]), ("mats", g_m[:bw.ml], ref["mats"])]
    worst = max(float(np.abs(g.astype(np.float64) - r).max()) / max(float(np.abs(r).max()), 1e-6) for _, g, r in pairs)
    claimed = [p for r, b, p in sc.claims_of(sc.BWD_PRED) if (r, b) == (name, B)]
    print("%s B=%d: loss %.6g (oracle %.6g), worst gradient error relative to its array's max %.3g; claims %s; "
          "stages %s" % (name, B, loss[0], ref["loss"], worst, claimed, sorted(stages)))
    assert abs(loss[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (name, B)
    for what, g, r in pairs:
        assert np.isfinite(g).all() and _close(g, r), (name, B, what)
    check_backward_stages(c, stages)
    check_claims(name, B, ncu, sc.BWD_PRED)
    if sc.wgrad_sq(B):  # the 208 x 208 dW's slice count is the restated one on this device's CU count
        for N, K, *_ in sc.wgrads(c):
            assert _lib.lib.rmx_debug_wgrad_slices(B, N, K, ncu) == sc.wgrad_sq_slices(B, N, K, ncu), (N, K, ncu)
    m.close()


def test_backward_cin_chunked_accumulating_dw(ctx):
    """wgrad_s3 0: the CIN's dW is no longer one launch over all B k rows with a generated operand -- every chunk
    of the CIN backward materialises z and its dW is added to the chunks before (wgrad's accum, r0 > 0).  B k =
    16,384 rows in chunks of 15,360: two, the second ragged.  Every gradient against the oracle at the usual bars,
    and the CIN weights against the default path within fp32 summation-order noise."""
    name, B = sc.CIN_ACCUM_RUN
    c = BY_NAME[name]
    assert sc.cin_rc_chunks(c, B) == 2
    m = sc.rmx_model(name)
    bw = backward_at(ctx, name, B)
    base = bw.run(m)
    rmx.set_tuning("wgrad_s3", 0)
    try:
        g_b, g_w, g_e, g_m, loss = bw.run(m)
    finally:
        rmx.set_tuning("wgrad_s3", None)
    ref = sc.oracle_backward(name, B)
    assert abs(loss[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    for what, g, r in (("bias", g_b, ref["bias"]), ("weights", g_w, ref["weights"]),
                       ("embedding", g_e, ref["embedding"]), ("mats", g_m[:bw.ml], ref["mats"])):
        err = float(np.abs(g.astype(np.float64) - r).max()) / max(float(np.abs(r).max()), 1e-6)
        print("%s B=%d wgrad_s3 0, %s: error relative to the array's max %.3g" % (name, B, what, err))
        assert np.isfinite(g).all() and _close(g, r), (name, B, what)
    d = float(np.abs(g_m - base[3]).max())
    assert d <= 1e-4 * float(np.abs(base[3]).max()), d
    m.close()


@pytest.mark.parametrize("name", sc.BWD_KNOB_ROWS)
def test_backward_knobs_agree(ctx, name):
    """The 208 x 208 dW against the 128 x 128 one (wgrad_sq 0) and the f32 MFMA one (wgrad_s3 0): fp32
    summation-order noise apart, 1e-4 of each array's maximum (test_train.py's bar between two dW kernels); the
    float4 slice reduction against the scalar one (slice_reduce4 0): the same sums in the same order, equal bits.
    That knob changes the kernels launched only where the float4 form runs (shape_cases.reduce_float4, head_float4:
    whole float4s written at 16-byte boundaries of mats): the dW and bias of dnn_f9k16_24x8x200x7x16's first three
    layers, layer 2 and the head's two passes of pnn_f7k10_33x20 -- dnn_f5k4_37x400 reduces everything scalar and is
    here for the dW kernels alone (test_ladder_reaches_every_path holds the knob rows to this)."""
    B = sc.B33K
    m = sc.rmx_model(name)
    bw = backward_at(ctx, name, B)
    base = bw.run(m)
    for knob, bitwise in (("wgrad_sq", False), ("wgrad_s3", False), ("slice_reduce4", True)):
        rmx.set_tuning(knob, 0)
        try:
            got = bw.run(m)
        finally:
            rmx.set_tuning(knob, None)
        for i, (a, b, wr) in enumerate(zip(base, got, bw.written)):
            if not wr:
                continue
            d = float(np.abs(a - b).max())
            print("%s %s 0, output %d: max |d| %.3g of max %.3g" % (name, knob, i, d, np.abs(a).max()))
            if bitwise:
                assert _same_bits(a, b), (name, knob, i)
            else:
                assert d <= 1e-4 * max(float(np.abs(a).max()), 1e-30), (name, knob, i)
    m.close()


@pytest.mark.parametrize("name", sc.BWD_LEFTOVER_ROWS)
def test_backward_leftovers(ctx, name):
    """The dX split GEMM's K tail (K = 7, 401) on the large-batch tiles reads dPre past K (zero_k_tail): primed at
    65,573, scratch and LDS filled with NaNs or ones, the five outputs keep the bits of the zero-filled run."""
    c = BY_NAME[name]
    B, big = sc.B33K, sc.FWD_LADDER[-1]
    m = sc.rmx_model(name)
    _Backward(ctx, c, big, sc.host_ids(c.F, big, 11)).run(m)
    bw = backward_at(ctx, name, B)
    kept = None
    for pat in (0, NAN, ONE):
        assert rmx.debug_poison_workspace(m, pat) > 0
        rmx.debug_fill_lds(ctx, pat)
        got = bw.run(m)
        if kept is None:
            kept = got
            assert all(np.isfinite(g).all() for g, wr in zip(kept, bw.written) if wr)
            assert _close(kept[3][:bw.ml], sc.oracle_backward(name, B)["mats"])
        for i, (g, k) in enumerate(zip(got, kept)):
            assert _same_bits(g, k), "%s backward output %d, pattern %s" % (name, i, hex(pat))
    m.close()
