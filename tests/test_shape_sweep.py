"""Every model off the benchmark shape (shape_cases.py) against the oracle: k != 16, odd tower widths, the
field counts at which a kernel changes, at B = 1, 37 and 300 (one partial block; two full 128-row blocks and a
ragged one).  The project's bars: |p - p_oracle| <= 1e-5 in fp32 (against the fp32 and the f64 oracle),
<= 2e-4 against the bf16 emulation on bf16-rounded parameters, test_train's bars for the gradients.
test_shape_sweep_cpu.py holds what makes a failure here the kernels': the oracle's own error is half the bar or
less, and dropping the edge column or unit of any layer moves p by 10 bars (fp32).  Each forward test also reads
the stage list, so that a row that stops reaching its kernels fails rather than passing on another path."""
import numpy as np
import pytest

import oracle_ctypes as oc
import rmx
import shape_cases as sc
from grad_check import _close
from shape_cases import BY_NAME, TOL, TOL_BF16, V

pytestmark = pytest.mark.gpu

NAN, ONE = 0x7FC07FC0, 0x3F803F80  # a NaN and ~1.0 in both the fp32 and the bf16 view of a word
BIAS_ARR = np.array([sc.BIAS], np.float32)


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


def _dev_ids(ctx, ids):
    return rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(ids, np.int32).reshape(-1))


def _forward_ids(ctx, m, t, B, ids_d):
    out = rmx.DeviceArray(ctx, B, np.float32)
    m.forward_ids(t, B, ids_d, out)
    ctx.sync()
    return out.numpy().copy()


def _forward_host(m, c, B, ids, bf16=False):
    """RecModel.forward on the caller's gathered fp32 arrays (never rounded: a bf16 model rounds them itself)."""
    w, e = sc.rows_of(c, ids)
    batch = (sc.index_of(B, c.F), np.asarray(ids, np.int64).reshape(-1))
    if c.kind == "lr":
        return m.forward(B, batch, BIAS_ARR, w)
    return m.forward(B, batch, BIAS_ARR, w, e, c.k, sc.host_mats(c.name, bf16), m.getMatsSize())


def _stages(m):
    names, _ = m.get_timing()
    return set(names)


def _check_stages(c, stages, bf16=False):
    """The stage list shows the path the row is in the table for."""
    def want(stage, on):
        assert (stage in stages) == bool(on), "%s: stage %s %s: %s" % (c.name, stage, "missing" if on else
                                                                         "not expected", sorted(stages))
    if c.kind == "lr":
        want("first_order_sigmoid", True)
        return
    want("gather_x", c.kind != "pnn" and sc.needs_gather_x(c.k, bf16))
    want("cross", c.kind == "dcn" and not sc.dcn_fused(c))
    want("product", c.kind == "pnn")
    want("cin_layer1", c.kind == "xdeepfm")
    # no row-owner kernel runs at these batches; DeepFM with k = 16 and two or more layers runs column-split
    # (the encoder stores x) at any F -- F = 40 and 41 alike
    want("tower_fused", False)
    want("tower_small", False)
    want("encoder_fm_x", not bf16 and sc.encoder_fm_x(c))
    want("tower_layer4+", len(c.fc) >= 4)


def _new_fp32(c):
    return sc.rmx_model(c.name)


# ---- forward, fp32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.NAMES)
def test_forward_ids_fp32(ctx, name):
    c = BY_NAME[name]
    m = _new_fp32(c)
    t = sc.dev_table(ctx, c.k)
    for B in sc.BATCHES:
        ids_d = _dev_ids(ctx, sc.host_ids(c.F, B))
        m.set_timing(True)
        got = _forward_ids(ctx, m, t, B, ids_d)
        stages = _stages(m)
        m.set_timing(False)
        e32 = float(np.abs(got - sc.oracle_forward(name, B, 0)).max())
        e64 = float(np.abs(got - sc.oracle_forward(name, B, 1)).max())
        print("%s B=%d: max |p - p32| = %.3g, max |p - p64| = %.3g, stages %s" % (name, B, e32, e64, sorted(stages)))
        assert np.isfinite(got).all()
        assert e32 <= TOL and e64 <= TOL, (name, B, e32, e64)
        again = _forward_ids(ctx, m, t, B, ids_d)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), (name, B, "a second launch differs")
        _check_stages(c, stages)


@pytest.mark.parametrize("name", sc.NAMES)
def test_forward_host_arrays_fp32(ctx, name):
    """RecModel.forward(batchSize, batch, bias, weights, embeddings, k, mats, matSizes): the reference's contract
    (no id array: the other branch of the gather, cross and product kernels)."""
    c = BY_NAME[name]
    m, m_ids = sc.rmx_model(name), _new_fp32(c)
    t = sc.dev_table(ctx, c.k)
    for B in sc.BATCHES:
        ids = sc.host_ids(c.F, B)
        got = _forward_host(m, c, B, ids)
        e32 = float(np.abs(got - sc.oracle_forward(name, B, 0)).max())
        e64 = float(np.abs(got - sc.oracle_forward(name, B, 1)).max())
        by_ids = _forward_ids(ctx, m_ids, t, B, _dev_ids(ctx, ids))
        d = float(np.abs(got - by_ids).max())
        print("%s B=%d: max |p - p32| = %.3g, max |p - p64| = %.3g, max |p - p(forward_ids)| = %.3g"
              % (name, B, e32, e64, d))
        assert got.shape == (B,) and np.isfinite(got).all()
        assert e32 <= TOL and e64 <= TOL, (name, B, e32, e64)
        # the same rows through the two entry points: equal bits, or fp32 summation order apart (the bar
        # test_gpu_parity.py holds between two paths of one batch)
        assert np.array_equal(got, by_ids) or d <= 2e-6, (name, B, d)


# ---- forward, bf16 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.BF16_NAMES)
def test_forward_bf16(ctx, name):
    c = BY_NAME[name]
    m = sc.rmx_model(name, bf16=True)
    t = sc.dev_table(ctx, c.k, bf16=True)
    if sc.bf16_refused(c):
        # a last hidden layer wider than one block has no bf16 kernel: a loud refusal, at every batch and
        # from both entry points, that leaves the library usable
        for B in sc.BATCHES:
            ids = sc.host_ids(c.F, B)
            with pytest.raises(rmx.RmxError):
                _forward_ids(ctx, m, t, B, _dev_ids(ctx, ids))
            with pytest.raises(rmx.RmxError):
                _forward_host(m, c, B, ids, bf16=True)
        B = 37
        got = _forward_ids(ctx, _new_fp32(c), sc.dev_table(ctx, c.k), B, _dev_ids(ctx, sc.host_ids(c.F, B)))
        assert float(np.abs(got - sc.oracle_forward(name, B, 1)).max()) <= TOL
        return
    for B in sc.BATCHES:
        ids = sc.host_ids(c.F, B)
        ref = sc.oracle_forward(name, B, 2, True)
        m.set_timing(True)
        got = _forward_ids(ctx, m, t, B, _dev_ids(ctx, ids))
        stages = _stages(m)
        m.set_timing(False)
        err = float(np.abs(got - ref).max())
        host = _forward_host(m, c, B, ids, bf16=True)  # unrounded fp32 arrays, rounded mats
        err_h = float(np.abs(host - ref).max())
        print("%s B=%d bf16: max |p - p_bf16 oracle| = %.3g (forward_ids), %.3g (host arrays), stages %s"
              % (name, B, err, err_h, sorted(stages)))
        assert np.isfinite(got).all() and np.isfinite(host).all()
        assert err <= TOL_BF16 and err_h <= TOL_BF16, (name, B, err, err_h)
        _check_stages(c, stages, bf16=True)


# ---- B = 65,536: the large-batch tile choice under a layer 1 gathered at k = 8 -----------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("name", sc.LARGE_NAMES)
def test_forward_large_batch(ctx, name, bf16):
    c = BY_NAME[name]
    B = sc.LARGE_B
    m = sc.rmx_model(name, bf16=bf16)
    t = sc.dev_table(ctx, c.k, bf16=bf16)
    ids_d = rmx.DeviceArray(ctx, B * c.F, np.int32)
    rmx.gen_ids(ctx, sc.SEED_IDS, 0, B, c.F, V, ids_d)
    got = _forward_ids(ctx, m, t, B, ids_d)
    assert np.isfinite(got).all()
    for r0, n in ((0, 512), (B - 300, 300)):  # the oracle on a head and a tail slice of the batch
        ids = oc.gen_ids(sc.SEED_IDS, r0, n, c.F, V)
        ref = sc.oracle_on(c, ids, 2 if bf16 else 1, bf16)
        err = float(np.abs(got[r0:r0 + n] - ref).max())
        print("%s B=%d bf16=%s rows %d..%d: max |p - p_oracle| = %.3g" % (name, B, bf16, r0, r0 + n, err))
        assert err <= (TOL_BF16 if bf16 else TOL), (name, r0, err)


@pytest.mark.parametrize("F", [40, 41])
def test_deepfm_field_limit_large_batch(ctx, F):
    """F = 40 is the last field count of the row-owner kernels and of the FM fused into layer 1 (kGMaxF, kFmMaxF):
    at the benchmark batch DeepFM 400-400-400 runs tower_fused at F = 40 and leaves it at F = 41."""
    name = "deepfm_f%dk16_400x400x400" % F
    c = BY_NAME[name]
    B = sc.LARGE_B
    m = _new_fp32(c)
    t = sc.dev_table(ctx, c.k)
    ids_d = rmx.DeviceArray(ctx, B * c.F, np.int32)
    rmx.gen_ids(ctx, sc.SEED_IDS, 0, B, c.F, V, ids_d)
    m.set_timing(True)
    got = _forward_ids(ctx, m, t, B, ids_d)
    stages = _stages(m)
    m.set_timing(False)
    print("%s B=%d: stages %s" % (name, B, sorted(stages)))
    if F == 40:
        assert stages == {"tower_fused"}, sorted(stages)
    else:  # no row-owner head (kGMaxF) and no FM fused into layer 1 (kFmMaxF): the encoder's FM, the gathered
        # layer 1 on the engine, then the row-owner tail, which takes no F
        assert stages == {"encoder_fm", "tower_layer1", "tower_tail"}, sorted(stages)
    for r0, n in ((0, 512), (B - 300, 300)):
        ref = sc.oracle_on(c, oc.gen_ids(sc.SEED_IDS, r0, n, c.F, V), 1)
        err = float(np.abs(got[r0:r0 + n] - ref).max())
        print("%s rows %d..%d: max |p - p64| = %.3g" % (name, r0, r0 + n, err))
        assert err <= TOL, (name, r0, err)


# ---- backward --------------------------------------------------------------------------------------------
class _Backward:
    """backward_ids on fixed ids / targets; the five outputs are NaN before every call."""

    def __init__(self, ctx, c, B, ids, bf16=False):
        self.ctx, self.c, self.B = ctx, c, B
        self.t = sc.dev_table(ctx, c.k, bf16)
        self.ids = _dev_ids(ctx, ids)
        self.targets = rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(sc.host_targets(B)))
        self.ml = len(sc.host_mats(c.name))
        sizes = (1, B * c.F, B * c.F * c.k, max(self.ml, 1), 1)
        self.outs = [rmx.DeviceArray(ctx, n, np.float32) for n in sizes]
        self.nans = [np.full(n, np.nan, np.float32) for n in sizes]
        self.written = (True, c.kind != "dnn", c.kind != "lr", c.kind != "lr", True)

    def run(self, m):
        for o, n in zip(self.outs, self.nans):
            o.upload(n)
        g = self.outs
        m.backward_ids(self.t, self.B, self.ids, self.targets, g[0], g[1], g[2], g[3] if self.ml else None, g[4])
        self.ctx.sync()
        return [o.numpy().copy() for o in self.outs]


@pytest.mark.parametrize("name", sc.NAMES)
def test_backward_ids(ctx, name):
    c = BY_NAME[name]
    m = _new_fp32(c)
    if sc.backward_refused(c):
        with pytest.raises(rmx.RmxError):
            _Backward(ctx, c, 37, sc.host_ids(c.F, 37)).run(m)
        return
    for B in (37, 300):
        bw = _Backward(ctx, c, B, sc.tie_free_ids(name, B))
        m.set_timing(True)
        g_b, g_w, g_e, g_m, loss = bw.run(m)
        stages = _stages(m)
        m.set_timing(False)
        ref = sc.oracle_backward(name, B)
        pairs = [(g_b, ref["bias"])] + ([(g_w, ref["weights"])] if c.kind != "dnn" else []) + \
            ([(g_e, ref["embedding"]), (g_m[:bw.ml], ref["mats"])] if c.kind != "lr" else [])
        worst = max(float(np.abs(g.astype(np.float64) - r).max()) / max(float(np.abs(r).max()), 1e-6) for g, r in pairs)
        print("%s B=%d: loss %.6g (oracle %.6g), worst gradient error relative to its array's max %.3g, stages %s"
              % (name, B, loss[0], ref["loss"], worst, sorted(stages)))
        assert abs(loss[0] - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (name, B)
        assert _close(g_b, ref["bias"]), (name, B, "bias")
        if c.kind != "dnn":
            assert _close(g_w, ref["weights"]), (name, B, "weights")
        if c.kind != "lr":
            assert _close(g_e, ref["embedding"]), (name, B, "embedding")
            assert _close(g_m[:bw.ml], ref["mats"]), (name, B, "mats")


@pytest.mark.parametrize("name", sc.BF16_NAMES)
def test_backward_bf16_refused(ctx, name):
    c = BY_NAME[name]
    m = sc.rmx_model(name, bf16=True)
    with pytest.raises(rmx.RmxError):
        _Backward(ctx, c, 37, sc.host_ids(c.F, 37), bf16=True).run(m)


# ---- leftovers -------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sc.NAMES)
def test_leftovers(ctx, name):
    """A pad column or a K tail that a 16-byte load reads past K is multiplied by a zero weight: harmless while
    the scratch holds finite leftovers, NaN once it holds one.  The model is primed at B = 300, so that its
    workspace is larger than the B = 37 calls; then the scratch in HBM and every CU's LDS are filled with a
    pattern before each call, and the outputs must keep their bits."""
    c = BY_NAME[name]
    B = 37
    m = _new_fp32(c)
    t = sc.dev_table(ctx, c.k)
    _forward_ids(ctx, m, t, 300, _dev_ids(ctx, sc.host_ids(c.F, 300, 11)))
    ids_d = _dev_ids(ctx, sc.host_ids(c.F, B))
    bw = None
    if not sc.backward_refused(c):
        _Backward(ctx, c, 300, sc.host_ids(c.F, 300, 11)).run(m)
        bw = _Backward(ctx, c, B, sc.tie_free_ids(name, B))

    def fill(pat):
        assert rmx.debug_poison_workspace(m, pat) > 0
        rmx.debug_fill_lds(ctx, pat)

    fill(0)
    kept = _forward_ids(ctx, m, t, B, ids_d)
    assert np.isfinite(kept).all()
    assert float(np.abs(kept - sc.oracle_forward(name, B, 1)).max()) <= TOL
    kept_b = None
    if bw:
        fill(0)
        kept_b = bw.run(m)
        for g, wr in zip(kept_b, bw.written):
            assert not wr or np.isfinite(g).all()
    for pat in (NAN, ONE):
        fill(pat)
        got = _forward_ids(ctx, m, t, B, ids_d)
        assert _same_bits(got, kept), "%s forward, pattern %s: max |d| %s" % (name, hex(pat), np.abs(got - kept).max())
        if bw:
            fill(pat)
            for i, (g, k) in enumerate(zip(bw.run(m), kept_b)):
                assert _same_bits(g, k), "%s backward output %d, pattern %s" % (name, i, hex(pat))


# ---- refusals and the PNN product kernel's LDS ----------------------------------------------------------
@pytest.mark.parametrize("make,words", [
    (lambda: rmx.DCN(V, 65, 16, 3, [16]), "1024"),                  # F k = 1,040
    (lambda: rmx.XDeepFM(V, 5, 8, [16], [8]), "16"),                # the CIN kernel's k
    (lambda: rmx.XDeepFM(V, 5, 16, [16], [257]), "256"),            # widest CIN tile + 1
    (lambda: rmx.PNN(V, 1, 16, [8]), "two fields"),
    (lambda: rmx.PNN(V, 640, 16, [8]), "10239"),                    # F k = 10,240: 16 (F k + 1) bytes > 160 KB
    (lambda: rmx.PNN(V, 2560, 4, [8]), "10239"),
])
def test_shapes_refused_at_creation(make, words):
    """Shapes no kernel holds fail when the model is made -- a host-side check: nothing is allocated on the
    device and nothing is launched."""
    live = rmx.debug_live_device_memory()
    with pytest.raises(rmx.RmxError) as ei:
        make()
    assert words in str(ei.value), str(ei.value)
    assert rmx.debug_live_device_memory() == live


def test_pnn_product_lds_at_the_limit(ctx):
    """F k = 10,239, the most that creation accepts: 16 (F k + 1) = 163,840 bytes, the whole LDS of a CU, as
    product_kernel's dynamic LDS (F = 3 fields of k = 3,413: three pairs, a small table), by ids and from host
    arrays, against the oracle at the fp32 bar."""
    F, k, fc, B, Vs = 3, 3413, (8,), 8, 64
    m = rmx.PNN(Vs, F, k, list(fc))
    om = oc.make_model(oc.PNN, F, k, fc=fc)
    mats = oc.init_mats(om, sc.SEED_MATS)
    m.setMats(mats)
    m.setBias(sc.BIAS)
    ids = oc.gen_ids(sc.SEED_IDS, 0, B, F, Vs)
    wt, et = oc.gen_table(sc.SEED_TAB, Vs, k)
    w, e = oc.gather(wt, et, 1, ids.astype(np.int64))
    t = rmx.EmbeddingTable(ctx, Vs, k)
    t.upload(wt, et)
    m.set_timing(True)
    got = _forward_ids(ctx, m, t, B, _dev_ids(ctx, ids))
    assert "product" in _stages(m)
    m.set_timing(False)
    ref = oc.forward(om, B, sc.index_of(B, F), BIAS_ARR, w, e, mats, 1)
    host = m.forward(B, (sc.index_of(B, F), ids.astype(np.int64)), BIAS_ARR, w, e, k, mats, m.getMatsSize())
    err, err_h = float(np.abs(got - ref).max()), float(np.abs(host - ref).max())
    print("PNN F=3 k=3413 (163,840 B of LDS): max |p - p64| = %.3g (forward_ids), %.3g (host arrays)" % (err, err_h))
    assert np.isfinite(ref).all() and err <= TOL and err_h <= TOL


def test_pnn_product_lds_above_64k(ctx):
    """PNN with F k = 4,160: the generic product kernel asks for 16 (F k + 1) = 66,576 bytes of dynamic LDS,
    more than a kernel is given unless the launch raises its limit first."""
    F, k, fc, B = 260, 16, (8,), 8
    m = rmx.PNN(V, F, k, list(fc))
    om = oc.make_model(oc.PNN, F, k, fc=fc)
    mats = oc.init_mats(om, sc.SEED_MATS)
    m.setMats(mats)
    m.setBias(sc.BIAS)
    ids = oc.gen_ids(sc.SEED_IDS, 0, B, F, V)
    wt, et = sc.host_table(k)
    w, e = oc.gather(wt, et, 1, ids.astype(np.int64))
    m.set_timing(True)
    got = _forward_ids(ctx, m, sc.dev_table(ctx, k), B, _dev_ids(ctx, ids))
    assert "product" in _stages(m)
    m.set_timing(False)
    for prec in (0, 1):
        ref = oc.forward(om, B, sc.index_of(B, F), BIAS_ARR, w, e, mats, prec)
        err = float(np.abs(got - ref).max())
        print("PNN F=260 k=16: max |p - p_oracle(precision %d)| = %.3g" % (prec, err))
        assert err <= TOL
    host = m.forward(B, (sc.index_of(B, F), ids.astype(np.int64)), BIAS_ARR, w, e, k, mats, m.getMatsSize())
    assert float(np.abs(host - ref).max()) <= TOL
