"""xDeepFM with a bf16 CIN (rmx_model_set_cin_precision(RMX_DTYPE_BF16), csrc/k_cin_bf16.hip) on the device.

The reference is tests/ref_cin_bf16.py: the fp64 model with the contract's two roundings (C_l to bf16; z = x0 u
formed in fp32 and rounded to bf16).  The CPU emulation puts the bf16 CIN's effect on p at initMats scale at
2-8e-6, below the 1e-5 bar, so a test on p alone cannot see a broken bf16 CIN; hence
  1. exact probes (every bf16 operation exact: the device must return the reference's bits);
  2. p against the rounded reference at the project's fp32 bar 1e-5 (what remains is fp32 accumulation, <= 1e-8);
  3. logit parity on test_logit_parity's scaled xDeepFM, bar e_trunc / 8 from the references alone
     (tests/test_cin_bf16_cpu.py::test_logit_reference_clearances);
  4-8. the fp32 path unchanged, every forward entry, the rejections, leftovers, memory.
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import ref_cin_bf16 as rc
import shape_cases as sc
import test_cin_bf16_cpu as cpu
import test_logit_parity as lp

pytestmark = pytest.mark.gpu

K = 16
TOL_P = 1e-5   # the project's fp32 bar on p (README "parity")
ULPS = 4       # of p, as tests/test_split_probes.py compares


@pytest.fixture(scope="module")
def ctx():
    import rmx
    return rmx.default_context()


def _bf16_model(make):
    import rmx
    m = make()
    m.setCinPrecision(rmx.DTYPE_BF16)
    assert m.getCinPrecision() == rmx.DTYPE_BF16
    return m


def _stages(m, fn):
    m.set_timing(True)
    fn()
    st, _ = m.get_timing()
    m.set_timing(False)
    return st


# ---- 1. exact probes ------------------------------------------------------------------------------------------
def test_probe_batches_claim_every_tile():
    seen = set()
    for Fn, cin in rc.PROBE_SHAPES:
        for B in rc.PROBE_BATCHES:
            seen.update(rc.cin_bf16_tiles(cin, B))
    assert seen == set(rc.ALL_TILES), seen


@pytest.mark.parametrize("Fn,cin", rc.PROBE_SHAPES)
def test_probes_exact(ctx, Fn, cin):
    import rmx
    wt, et = rc.probe_table()
    table = rmx.EmbeddingTable(ctx, rc.PROBE_V, K)
    table.upload(wt, et)
    m = _bf16_model(lambda: rmx.XDeepFM(rc.PROBE_V, Fn, K, list(rc.PROBE_FC), list(cin)))
    m.setBias(rc.PROBE_BETA)
    Bmax = max(rc.PROBE_BATCHES)
    ids = rc.probe_ids(Fn, Bmax)
    ids_d = rmx.DeviceArray.from_numpy(ctx, ids.ravel())
    out = rmx.DeviceArray(ctx, Bmax, np.float32)
    for rnd in range(rc.probe_rounds(cin)):
        m.setMats(rc.probe_mats(Fn, cin, rnd))
        for B in rc.PROBE_BATCHES:  # (the first B rows of the same ids)
            rows = rc.rows_of(B)
            want = rc.sigmoid32(rc.probe_expected(Fn, cin, ids[rows], rnd))
            m.forward_ids(table, B, ids_d, out)
            ctx.sync()
            got = out.numpy()[:B]
            assert np.isfinite(got).all()
            err = np.abs(got[rows].astype(np.float64) - want)
            bad = np.flatnonzero(~(err <= ULPS * np.spacing(want).astype(np.float64)))
            assert bad.size == 0, "F=%d cin=%s round %d B=%d tiles %s: rows %s: p %s, expected %s" % (
                Fn, cin, rnd, B, rc.cin_bf16_tiles(cin, B), rows[bad][:6], got[rows][bad][:6], want[bad][:6])
    m.close()


# ---- 2. p against the rounded reference ---------------------------------------------------------------------
XDEEPFM_ROWS = [c.name for c in sc.CASES if c.kind == "xdeepfm"]
P_CASES = [(n, B) for n in XDEEPFM_ROWS for B in (517, 4099)]


def _reference_p(c, ids, mats, **kw):
    ids = np.asarray(ids).reshape(-1, c.F)
    n = ids.shape[0]
    w, e = sc.rows_of(c, ids)
    return rc.forward(n, c.F, c.k, sc.index_of(n, c.F), np.array([sc.BIAS], np.float32), w, e, mats, c.fc, c.cin, **kw)


def test_the_shape_rows_are_the_four_xdeepfm_entries():
    assert len(XDEEPFM_ROWS) == 4


@pytest.mark.parametrize("name,B", P_CASES)
def test_p_parity_shape_rows(ctx, name, B):
    import rmx
    c = sc.BY_NAME[name]
    m = sc.rmx_model(name)
    m.setCinPrecision(rmx.DTYPE_BF16)
    m.setMats(sc.host_mats(name))
    ids = sc.host_ids(c.F, B)
    ids_d = rmx.DeviceArray.from_numpy(ctx, ids)
    out = rmx.DeviceArray(ctx, B, np.float32)
    st = _stages(m, lambda: (m.forward_ids(sc.dev_table(ctx, c.k), B, ids_d, out), ctx.sync()))
    assert "cin_layer1" in st
    rows = rc.rows_of(B)
    got = out.numpy()[rows]
    sel = ids.reshape(B, c.F)[rows]
    ref = _reference_p(c, sel, sc.host_mats(name))
    unrounded = sc.oracle_on(c, sel, 1)
    err = float(np.abs(got - ref).max())
    print("%s B=%d bf16 CIN (%s): max|p - p_ref| = %.3g, max|p - p_fp64(unrounded)| = %.3g" % (
        name, B, rc.cin_bf16_tiles(c.cin, B), err, float(np.abs(got - unrounded).max())))
    assert err <= TOL_P
    m.close()


FLAG = dict(F=39, fc=(400, 400, 400), cin=(200, 200, 200), V=50000, B=517)


def test_p_parity_flagship_shape(ctx):
    import rmx
    f = FLAG
    m = _bf16_model(lambda: rmx.XDeepFM(f["V"], f["F"], K, list(f["fc"]), list(f["cin"])))
    mats = m.initMats(lp.SEED_MATS)
    m.setMats(mats)
    m.setBias(0.01)
    table = rmx.EmbeddingTable(ctx, f["V"], K)
    table.fill_synthetic(lp.SEED_TAB)
    B = f["B"]
    ids = oc.gen_ids(lp.SEED_IDS, 0, B, f["F"], f["V"]).astype(np.int32)
    ids_d = rmx.DeviceArray.from_numpy(ctx, ids)
    out = rmx.DeviceArray(ctx, B, np.float32)
    m.forward_ids(table, B, ids_d, out)
    ctx.sync()
    rows = rc.rows_of(B)
    wt, et = oc.gen_table(lp.SEED_TAB, f["V"], K)
    flat = ids.reshape(B, f["F"])[rows].astype(np.int64).ravel()
    w, e = oc.gather(wt, et, 1, flat)
    n = rows.size
    args = (n, f["F"], K, np.repeat(np.arange(n, dtype=np.int64), f["F"]), np.array([0.01], np.float32), w, e, mats,
            f["fc"], f["cin"])
    ref = rc.forward(*args)
    unrounded = rc.forward(*args, round_w=False, round_z=None)
    got = out.numpy()[rows]
    err = float(np.abs(got - ref).max())
    print("xdeepfm F=39 400^3 cin 200^3 B=%d bf16 CIN: max|p - p_ref| = %.3g, max|p - p_fp64(unrounded)| = %.3g" % (
        B, err, float(np.abs(got - unrounded).max())))
    assert err <= TOL_P
    m.close()


# ---- 3. logit parity where the CIN is visible -------------------------------------------------------------
@pytest.mark.parametrize("B", cpu.LOGIT_BATCHES)
def test_logit_parity(ctx, B):
    """max |logit(gpu) - logit(reference)| <= e_trunc / 8 over the rows with reference p in [0.02, 0.98].
    Measured on an MI355X: see DESIGN.md (bf16 CIN)."""
    import rmx
    r = cpu.logit_refs(B)
    m = _bf16_model(lambda: lp._model("xdeepfm"))
    m.setMats(lp.scaled_mats("xdeepfm"))
    m.setBias(lp.BETA)
    table = rmx.EmbeddingTable(ctx, lp.V, K)
    table.fill_synthetic(lp.SEED_TAB)
    ids = rmx.DeviceArray(ctx, B * lp.F, np.int32)
    rmx.gen_ids(ctx, lp.SEED_IDS, 0, B, lp.F, lp.V, ids)
    out = rmx.DeviceArray(ctx, B, np.float32)
    st = _stages(m, lambda: (m.forward_ids(table, B, ids, out), ctx.sync()))
    assert "cin_layer2" in st
    p = out.numpy()[r["rows"]]
    assert np.isfinite(p).all()
    e = float(np.abs(rc.logit(p) - r["l_ref"])[r["keep"]].max())
    print("xdeepfm B=%d bf16 CIN (%s): max|logit - logit_ref| = %.3g  (e_acc %.3g, e_trunc %.3g, bar %.3g)" % (
        B, rc.cin_bf16_tiles((200, 200), B), e, r["e_acc"], r["e_trunc"], r["e_trunc"] / 8))
    assert e <= r["e_trunc"] / 8
    m.close()


# ---- 4. nothing else moved --------------------------------------------------------------------------------
def test_fp32_forward_is_unchanged_around_a_switch(ctx):
    import rmx
    name = "xdeepfm_f5k16_33_cin200x7"
    c = sc.BY_NAME[name]
    B = 517
    ids_d = rmx.DeviceArray.from_numpy(ctx, sc.host_ids(c.F, B))
    out = rmx.DeviceArray(ctx, B, np.float32)
    table = sc.dev_table(ctx, c.k)

    def run(m):
        m.forward_ids(table, B, ids_d, out)
        ctx.sync()
        return out.numpy().copy()

    m = sc.rmx_model(name)
    before = run(m)
    m.setCinPrecision(rmx.DTYPE_F32)  # the current value: nothing happens, the parameters stay loaded
    assert np.array_equal(run(m), before)
    m.setCinPrecision(rmx.DTYPE_BF16)
    with pytest.raises(rmx.RmxError):  # the switch dropped the parameters
        run(m)
    m.setMats(sc.host_mats(name))
    assert np.isfinite(run(m)).all()
    assert np.array_equal(m.getMats(), sc.host_mats(name))  # the caller's fp32 values, not the rounded ones
    m.setCinPrecision(rmx.DTYPE_F32)
    assert m.getCinPrecision() == rmx.DTYPE_F32
    m.setMats(sc.host_mats(name))
    assert np.array_equal(run(m), before)
    assert np.array_equal(run(sc.rmx_model(name)), before)
    with pytest.raises(rmx.RmxError):
        m.setPrecision(rmx.DTYPE_BF16)
    m.close()


# ---- 5. every forward entry -------------------------------------------------------------------------------
def test_every_forward_entry(ctx):
    import rmx
    name = "xdeepfm_f5k16_33_cin200x7"
    c = sc.BY_NAME[name]
    m = sc.rmx_model(name)
    m.setCinPrecision(rmx.DTYPE_BF16)
    m.setMats(sc.host_mats(name))
    table = sc.dev_table(ctx, c.k)
    N, step = 1000, 300
    ids = sc.host_ids(c.F, N)
    ids_d = rmx.DeviceArray.from_numpy(ctx, ids)
    scores = rmx.DeviceArray(ctx, N, np.float32)
    m.predict_ids(table, N, ids_d, scores, batch=step)
    ctx.sync()
    pred = scores.numpy().copy()
    fwd = np.zeros(N, np.float32)
    for r0 in range(0, N, step):
        n = min(step, N - r0)
        part_d = rmx.DeviceArray.from_numpy(ctx, ids.reshape(N, c.F)[r0:r0 + n].ravel())
        out = rmx.DeviceArray(ctx, n, np.float32)
        m.forward_ids(table, n, part_d, out)
        ctx.sync()
        fwd[r0:r0 + n] = out.numpy()
    assert np.array_equal(pred, fwd)
    # L-A: host arrays
    B = 300
    sel = ids.reshape(N, c.F)[:B]
    w, e = sc.rows_of(c, sel)
    got = m.forward(B, (sc.index_of(B, c.F), sel.astype(np.int64).ravel()), np.array([sc.BIAS], np.float32), w, e,
                    c.k, sc.host_mats(name), m.getMatsSize())
    rows = rc.rows_of(B)
    ref = _reference_p(c, sel[rows], sc.host_mats(name))
    assert np.abs(got[rows] - ref).max() <= TOL_P
    assert np.array_equal(got, fwd[:B])
    # a 2-rank loopback shard holding the same rows
    shard = rmx.ShardedTable(ctx, sc.V, c.k, 2)
    shard.fill_synthetic(sc.SEED_TAB)
    out = rmx.DeviceArray(ctx, step, np.float32)
    part_d = rmx.DeviceArray.from_numpy(ctx, ids.reshape(N, c.F)[:step].ravel())
    m.forward_ids_sharded(shard, step, part_d, out)
    ctx.sync()
    assert np.array_equal(out.numpy(), fwd[:step])
    shard.pull(part_d, step * c.F, 0)
    m.forward_pulled(shard, step, 0, out)
    ctx.sync()
    assert np.array_equal(out.numpy(), fwd[:step])
    m.close()


# ---- 6. rejections ----------------------------------------------------------------------------------------
def test_backward_and_optimisers_are_rejected(ctx):
    import rmx
    from rmx import _lib
    name = "xdeepfm_f5k16_100x37_cin10x7"
    c = sc.BY_NAME[name]
    B = 37
    table = sc.dev_table(ctx, c.k)
    shard = rmx.ShardedTable(ctx, sc.V, c.k, 2)
    shard.fill_synthetic(sc.SEED_TAB)
    m = sc.rmx_model(name)
    opt = rmx.Optimizer(m, table, "sgd", eta=0.1)          # made while the CIN is fp32
    sopt = rmx.Optimizer(m, shard, "sgd", eta=0.1)
    m.setCinPrecision(rmx.DTYPE_BF16)
    m.setMats(sc.host_mats(name))
    ids = sc.host_ids(c.F, B)
    ids_d = rmx.DeviceArray.from_numpy(ctx, ids)
    tg_d = rmx.DeviceArray.from_numpy(ctx, sc.host_targets(B))
    w, e = sc.rows_of(c, ids)
    mats = np.array(sc.host_mats(name))
    shard.pull(ids_d, B * c.F, 0)
    ctx.sync()

    calls = {
        "rmx_backward": lambda: m.backward(B, (sc.index_of(B, c.F), ids.astype(np.int64)), np.array([sc.BIAS], np.float32),
                                           np.array(w), np.array(e), c.k, mats, m.getMatsSize(), sc.host_targets(B)),
        "rmx_backward_ids": lambda: m.backward_ids(table, B, ids_d, tg_d),
        "rmx_backward_pulled": lambda: m.backward_pulled(shard, B, 0, tg_d),
        "rmx_optim_create": lambda: rmx.Optimizer(m, table, "sgd", eta=0.1),
        "rmx_optim_create_sharded": lambda: rmx.Optimizer(m, shard, "sgd", eta=0.1),
        "rmx_train_step_ids": lambda: m.train_step_ids(table, opt, B, ids_d, tg_d),
        "rmx_train_step_sharded": lambda: m.train_step_sharded(shard, sopt, B, ids_d, tg_d),
    }
    for who, call in calls.items():
        live = rmx.debug_live_device_memory()
        with pytest.raises(rmx.RmxError) as ei:
            call()
        assert ei.value.code == _lib.RMX_E_INVALID, who
        assert "rmx_model_set_cin_precision" in str(ei.value) and who in str(ei.value), (who, str(ei.value))
        assert rmx.debug_live_device_memory() == live, who
    out = rmx.DeviceArray(ctx, B, np.float32)
    m.forward_pulled(shard, B, 0, out)  # the pull the rejected backward left is still there to consume
    ctx.sync()
    assert np.isfinite(out.numpy()).all()
    opt.close()   # (the optimisers hold the model: they go first)
    sopt.close()
    m.close()


def test_set_cin_precision_rejects_other_models_and_dtypes(ctx):
    import rmx
    from rmx import _lib
    V, F = 100, 4
    others = [rmx.DeepFM(V, F, K, [8]), rmx.DCN(V, F, K, 2, [8, 8]), rmx.PNN(V, F, K, [8]), rmx.DNN(V, F, K, [8]),
              rmx.LR(V, F)]
    for m in others:
        m._device()
        live = rmx.debug_live_device_memory()
        with pytest.raises(rmx.RmxError) as ei:
            m.setCinPrecision(rmx.DTYPE_BF16)
        assert ei.value.code == _lib.RMX_E_INVALID and "xDeepFM" in str(ei.value)
        assert rmx.debug_live_device_memory() == live
        assert m.getCinPrecision() == rmx.DTYPE_F32
    x = rmx.XDeepFM(V, F, K, [8], [8])
    for bad in (-1, 2, 7):
        with pytest.raises(rmx.RmxError) as ei:
            x.setCinPrecision(bad)
        assert ei.value.code == _lib.RMX_E_INVALID and "dtype" in str(ei.value)
    assert x.getCinPrecision() == rmx.DTYPE_F32
    assert _lib.lib.rmx_model_set_cin_precision(None, rmx.DTYPE_BF16) == _lib.RMX_E_INVALID


# ---- 7. leftovers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (37, 517))
def test_lds_and_workspace_leftovers(ctx, B):
    """A NaN pattern in every CU's LDS and in the model's workspace (the maps' pad columns 200..207, the rows past
    M of a ragged block) must not reach the output."""
    import rmx
    m = _bf16_model(lambda: lp._model("xdeepfm"))
    m.setMats(lp.scaled_mats("xdeepfm"))
    m.setBias(lp.BETA)
    table = rmx.EmbeddingTable(ctx, lp.V, K)
    table.fill_synthetic(lp.SEED_TAB)
    ids = rmx.DeviceArray(ctx, B * lp.F, np.int32)
    rmx.gen_ids(ctx, lp.SEED_IDS, 0, B, lp.F, lp.V, ids)
    out = rmx.DeviceArray(ctx, B, np.float32)
    m.forward_ids(table, B, ids, out)
    ctx.sync()
    first = out.numpy().copy()
    assert np.isfinite(first).all()
    rmx.debug_fill_lds(ctx, 0x7FC00000)
    assert rmx.debug_poison_workspace(m) > 0
    m.forward_ids(table, B, ids, out)
    ctx.sync()
    assert np.array_equal(out.numpy(), first)
    m.close()


# ---- 8. memory --------------------------------------------------------------------------------------------
def test_device_memory_returns(ctx):
    import rmx
    name = "xdeepfm_f5k16_33_cin200x7"
    c = sc.BY_NAME[name]
    B = 37
    table = sc.dev_table(ctx, c.k)
    ids_d = rmx.DeviceArray.from_numpy(ctx, sc.host_ids(c.F, B))
    out = rmx.DeviceArray(ctx, B, np.float32)
    ctx.sync()
    first = rmx.debug_live_device_memory()
    m = rmx.XDeepFM(sc.V, c.F, c.k, list(c.fc), list(c.cin))
    m._device()
    f32_bytes = rmx.debug_live_device_memory()[0]
    m.setCinPrecision(rmx.DTYPE_BF16)
    assert rmx.debug_live_device_memory()[0] < f32_bytes  # the fp32 CIN forms are dropped
    m.setMats(sc.host_mats(name))
    m.setBias(sc.BIAS)
    m.forward_ids(table, B, ids_d, out)
    ctx.sync()
    m.setCinPrecision(rmx.DTYPE_F32)
    m.setMats(sc.host_mats(name))
    m.forward_ids(table, B, ids_d, out)
    ctx.sync()
    m.close()
    assert rmx.debug_live_device_memory() == first
