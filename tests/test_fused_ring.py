"""GPU parity of the fused fp32 tower's weight ring when it is validated one unit ahead (csrc/k_fused_s3.hip,
k_rowown.hpp q_unit_ring): the barrier at the head of unit U proves unit U + 1 as well, so a wave prefetches
the next unit's first weight fragments before it reaches the barrier.  A fragment read of a slot that no
barrier has proven, a wrong static vmcnt or a wrong phase of the carried fragment registers gives wrong
bits, not a fault -- so every case here is BITWISE against head + tail (knob s3_fused 2 vs 0 with s3_head and
s3_tail forced on, as test_fused_s3.py does), within 1e-5 of the fp64 oracle on a strided sample of at most
512 rows, and run twice for equal bits.

Cases: field counts 3, 5 and 6 (KS = 2, 3, 3 layer-1 K steps; with test_fused_s3.py's 1, 2, 7, 39 and 40 every
remainder of KS modulo 3 is covered), each at B = 33,000 (a full row block followed by a half block on the
same CU) and at B = 65,536 + 384 (some CUs run three row blocks); F = 39 at B = 128 and 129 (one row block, and
one plus a ragged half block: the ring starts and ends inside a block, with units past the end DMA'd but never
computed); and F = 39 at B = 65,537 after every CU's LDS was filled with NaN."""
import numpy as np
import pytest

import oracle_ctypes as oc
import rmx

pytestmark = pytest.mark.gpu

TOL = 1e-5
K, V = 16, 50_000
SEED_IDS, SEED_TAB, SEED_MATS = 0xF05E, 0x7AB1E, 0x3A75
FC = (400, 400, 400)
_TABLE = {}


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(autouse=True)
def _restore_knobs():
    rmx.set_tuning("s3_small", 0)  # (small batches would run the whole-tower kernel, k_small_s3.hip)
    yield
    for k in ("s3_fused", "s3_head", "s3_tail", "s3_small"):
        rmx.set_tuning(k, None)


def _oracle_table():
    if not _TABLE:
        _TABLE["t"] = oc.gen_table(SEED_TAB, V, K)  # computed once, read by every case
    return _TABLE["t"]


def _fwd(ctx, m, table, B, ids, out, fused, fill=None):
    rmx.set_tuning("s3_fused", 2 if fused else 0)
    rmx.set_tuning("s3_head", 2)
    rmx.set_tuning("s3_tail", 2)
    if fill is not None:
        rmx.debug_fill_lds(ctx, fill)
    m.set_timing(True)
    m.forward_ids(table, B, ids, out)
    ctx.sync()
    stages, _ = m.get_timing()
    m.set_timing(False)
    assert ("tower_fused" in stages) == fused, stages
    return out.numpy().copy()


def _check(ctx, Fn, B, fill=None):
    m = rmx.DeepFM(V, Fn, K, list(FC))
    mats = m.initMats(SEED_MATS)
    m.setMats(mats)
    m.setBias(0.01)
    table = rmx.EmbeddingTable(ctx, V, K)
    table.fill_synthetic(SEED_TAB)
    ids = rmx.DeviceArray(ctx, B * Fn, np.int32)
    rmx.gen_ids(ctx, SEED_IDS, 0, B, Fn, V, ids)
    out = rmx.DeviceArray(ctx, B, np.float32)
    got = _fwd(ctx, m, table, B, ids, out, True, fill)
    ref = _fwd(ctx, m, table, B, ids, out, False)
    assert np.isfinite(got).all()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, "%d rows differ from head + tail (first %s, max |d| %.3g)" % (
        bad.size, bad[:8].tolist(), float(np.abs(got - ref).max()))
    # the fp64 oracle on a strided sample (at most 512 rows, the last row among them)
    rows = np.union1d(np.arange(0, B, -(-B // 500)), [B - 1])
    assert rows.size <= 512
    wt, et = _oracle_table()
    om = oc.make_model(oc.DEEPFM, Fn, K, fc=FC)
    h = oc.gen_ids(SEED_IDS, 0, B, Fn, V).reshape(B, Fn)[rows].astype(np.int64).ravel()
    w, e = oc.gather(wt, et, 1, h)
    n = rows.size
    r64 = oc.forward(om, n, np.repeat(np.arange(n, dtype=np.int64), Fn), np.array([0.01], np.float32), w, e, mats, 1)
    e64 = float(np.abs(got[rows] - r64).max())
    print("F=%d B=%d: fused == head + tail; %d rows vs fp64 %.3g" % (Fn, B, n, e64))
    assert e64 <= TOL
    # deterministic: a second run gives the same bits
    assert np.array_equal(_fwd(ctx, m, table, B, ids, out, True, fill), got)


@pytest.mark.parametrize("B", [33000, 65536 + 384])
@pytest.mark.parametrize("Fn", [3, 5, 6])
def test_ring_field_counts(ctx, Fn, B):
    """KS = 2, 3, 3 layer-1 K steps; a full block then a half block on one CU (33,000), three row blocks on some
    CUs (65,920)."""
    _check(ctx, Fn, B)


@pytest.mark.parametrize("B", [128, 129])
def test_ring_single_row_block(ctx, B):
    """One row block (128) and one plus a ragged half block of one row (129): the ring starts and ends inside a
    block; the units DMA'd past its end are never read."""
    _check(ctx, 39, B)


def test_ring_after_nan_lds(ctx):
    """Every CU's LDS holds NaN before the launch: a fragment read of a slot that no barrier has proven would
    feed NaN into the MFMAs."""
    _check(ctx, 39, 65537, fill=0x7FC00000)
