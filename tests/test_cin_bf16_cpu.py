"""The bf16 CIN's references, checked on the CPU (tests/test_cin_bf16.py runs the device against them).

  * ref_cin_bf16.forward with both roundings off is ref_numpy.forward: the same model;
  * the C API of rmx_model_set_cin_precision on a host-only model;
  * the exact probes are exact: every z and weight is a bf16 value, fp32 sums in a scrambled order equal the fp64
    sums bit for bit, every u, pool and logit is an fp32 value;
  * the logit test's bar e_trunc / 8 (z cut toward zero instead of rounded, the nearest wrong arithmetic) leaves
    honest fp32 accumulation 4x room, and the reference alone meets the exclusion cap and the visibility rule.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle_ctypes as oc
import ref_cin_bf16 as rc
import ref_numpy
import test_logit_parity as lp

F, K = 39, 16


def test_helper_without_roundings_is_ref_numpy():
    rng = np.random.default_rng(3)
    for Fn, fc, cin in ((5, (33,), (10, 7)), (7, (12, 9), (20,))):
        B = 9
        om = oc.make_model(oc.XDEEPFM, Fn, K, fc=fc, cin=cin)
        mats = oc.init_mats(om, 5)
        index = np.repeat(np.arange(B, dtype=np.int64), Fn)
        w = rng.uniform(-0.05, 0.05, B * Fn).astype(np.float32)
        e = rng.uniform(-0.05, 0.05, B * Fn * K).astype(np.float32)
        bias = np.array([0.01], np.float32)
        want = ref_numpy.forward("xdeepfm", B, Fn, K, index, bias, w, e, mats, fc=fc, cin=cin)
        got = rc.forward(B, Fn, K, index, bias, w, e, mats, fc, cin, round_w=False, round_z=None)
        assert np.abs(got - want).max() <= 1e-15
        # ... and the roundings do something
        assert np.abs(rc.forward(B, Fn, K, index, bias, w, e, mats, fc, cin) - want).max() > 0


def test_cin_precision_api_on_a_host_only_model():
    """Fails without the feature: the symbols do not exist."""
    import rmx
    from rmx import _lib
    lib = _lib.lib
    assert hasattr(lib, "rmx_model_set_cin_precision") and hasattr(lib, "rmx_model_get_cin_precision")
    m = rmx.XDeepFM(1000, 5, K, [8], [8])
    assert m.getCinPrecision() == rmx.DTYPE_F32  # host-only handle: no GPU touched
    assert lib.rmx_model_get_cin_precision(m._meta) == rmx.DTYPE_F32
    assert lib.rmx_model_get_cin_precision(None) < 0
    lib.rmx_last_error.restype = ctypes.c_char_p
    st = lib.rmx_model_set_cin_precision(m._meta, rmx.DTYPE_BF16)
    assert st == _lib.RMX_E_INVALID
    msg = lib.rmx_last_error().decode()
    assert "rmx_model_set_cin_precision" in msg and "host-only" in msg
    st = lib.rmx_model_set_cin_precision(None, rmx.DTYPE_BF16)
    assert st == _lib.RMX_E_INVALID
    msg = lib.rmx_last_error().decode()
    assert "rmx_model_set_cin_precision" in msg and "NULL" in msg
    assert lib.rmx_model_get_cin_precision(m._meta) == rmx.DTYPE_F32


def test_tile_mirror_claims():
    """The batches of the probe test reach every tile of the bf16 selection."""
    seen = set()
    for Fn, cin in rc.PROBE_SHAPES:
        for B in rc.PROBE_BATCHES:
            seen.update(rc.cin_bf16_tiles(cin, B))
    assert seen == set(rc.ALL_TILES), seen


@pytest.mark.parametrize("Fn,cin", rc.PROBE_SHAPES)
def test_probes_are_exact(Fn, cin):
    B = 48
    ids = rc.probe_ids(Fn, B)
    rng = np.random.default_rng(9)
    for rnd in range(rc.probe_rounds(cin)):
        dt = {}
        lg = rc.probe_expected(Fn, cin, ids, rnd, dt)
        for Z, W in zip(dt["z"], dt["w"]):
            z32 = Z.astype(np.float32)
            assert np.array_equal(z32.astype(np.float64), Z)
            assert np.array_equal(oc.round_bf16(z32), z32), "a z is no bf16 value"
            assert np.array_equal(rc.trunc_bf16(z32), z32)
            if rnd:
                continue  # (the CIN weights are the same in every round)
            w32 = W.astype(np.float32)
            assert np.array_equal(oc.round_bf16(w32), w32), "a weight is no bf16 value"
            # fp32 accumulation, one product at a time, in a scrambled K order == the fp64 sum, bit for bit
            perm = rng.permutation(Z.shape[1])
            rows = rng.choice(Z.shape[0], size=8, replace=False)
            a = np.zeros((rows.size, W.shape[0]), np.float32)
            for kk in perm:
                a = a + np.outer(z32[rows, kk], w32[:, kk]).astype(np.float32)
            assert np.array_equal(a.astype(np.float64), Z[rows] @ W.T)
        if rnd == 0:
            # the weights as given in mats are the rounded ones: the packed plane holds them unchanged
            lay, _, _ = rc.probe_layout(Fn, cin)
            mats = rc.probe_mats(Fn, cin, 0)
            for (c0, b0, hp, h) in lay:
                assert np.array_equal(oc.round_bf16(mats[c0:b0]), mats[c0:b0])
        for a in dt["u"] + dt["pools"] + [lg]:
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "not an fp32 value"
        # the rowdot, the sum over the layers and the pooling, in any order: every term u * w_out is a multiple of
        # 2^-17 (u of 2^-11, w_out +-2^-4 .. 2^-6) and the sum of their magnitudes stays below 2^7: 24 bits
        lay, wo_off, _ = rc.probe_layout(Fn, cin)
        mats = rc.probe_mats(Fn, cin, rnd)
        tot, base = 0.0, 0
        for u, (_, _, _, h) in zip(dt["u"], lay):
            assert np.array_equal(u * 2 ** 11, np.round(u * 2 ** 11))
            wo = np.abs(mats[wo_off + base:wo_off + base + h].astype(np.float64))
            assert set(np.unique(wo)) <= {0.0, 2.0 ** -4, 2.0 ** -5, 2.0 ** -6}
            tot = tot + (np.abs(u).reshape(B, K, h).sum(axis=1) * wo).sum(axis=1)
            base += h
        assert tot.max() < 2 ** 7
        # visible: the logit moves with the CIN, and stays where one step of it (2^-17: one z * C term of 2^-11
        # under the smallest output weight) moves p by twice the 4 ulps the device test allows
        print("F=%d cin=%s round %d: logit in [%.3f, %.3f], %d distinct of %d" % (Fn, cin, rnd, lg.min(), lg.max(),
                                                                                  np.unique(lg).size, B))
        assert np.unique(lg).size > B // 2
        p = rc.sigmoid32(lg).astype(np.float64)
        assert (2.0 ** -17 * p * (1 - p) >= 2 * 4 * np.spacing(p.astype(np.float32))).all()


# ---- the logit test's references ------------------------------------------------------------------------
LOGIT_KIND = "xdeepfm"
LOGIT_BATCHES = (300, 4099)


@functools.lru_cache(None)
def logit_refs(B):
    """On at most 64 rows of test_logit_parity's xDeepFM case: the reference logit, e_trunc and e_acc (computed
    once, shared read-only with tests/test_cin_bf16.py)."""
    kw = lp.CASES[LOGIT_KIND]["kw"]
    om, rows512, n512, index512, bias, w512, e512 = lp.inputs(LOGIT_KIND, B)
    sel = rc.rows_of(n512)          # 64 of the case's oracle rows
    rows = rows512[sel]
    n = sel.size
    w = w512.reshape(n512, F)[sel].ravel()
    e = e512.reshape(n512, F * K)[sel].ravel()
    index = np.repeat(np.arange(n, dtype=np.int64), F)
    mats = lp.scaled_mats(LOGIT_KIND)
    run = lambda **k_: rc.forward(n, F, K, index, bias, w, e, mats, kw["fc"], kw["cin"], **k_)
    p_ref = run()
    l_ref = rc.logit(p_ref)
    keep = (p_ref >= lp.P_LO) & (p_ref <= lp.P_HI)
    e_trunc = float(np.abs(rc.logit(run(round_z="trunc")) - l_ref)[keep].max())
    e_acc = float(np.abs(rc.logit(run(acc="fp32").astype(np.float32)) - l_ref)[keep].max())
    m0 = np.array(mats)
    m0[lp._out_slice(LOGIT_KIND, m0.size)] = 0
    part = l_ref - rc.logit(rc.forward(n, F, K, index, bias, w, e, m0, kw["fc"], kw["cin"]))
    res = dict(rows=rows, keep=keep, l_ref=l_ref, e_trunc=e_trunc, e_acc=e_acc, part=part)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@pytest.mark.parametrize("B", LOGIT_BATCHES)
def test_logit_reference_clearances(B):
    r = logit_refs(B)
    print("xdeepfm B=%d: e_trunc %.3g (bar %.3g), e_acc %.3g; excluded %d of %d; std part %.3g of logit %.3g" % (
        B, r["e_trunc"], r["e_trunc"] / 8, r["e_acc"], (~r["keep"]).sum(), r["keep"].size, r["part"].std(),
        r["l_ref"].std()))
    assert r["e_trunc"] / 8 >= 4 * r["e_acc"]
    assert (~r["keep"]).mean() <= lp.MAX_EXCLUDED
    assert np.isfinite(r["l_ref"]).all()
    assert r["part"].std() >= 0.5 * r["l_ref"].std()
