"""Every device buffer of librmx belongs to an object and leaves with it: rmx_debug_live_device_memory (live
bytes, live buffers of the whole process) is strictly larger while a model, table, optimiser or shard lives and
is back at its earlier reading, exactly, once they are destroyed.

The shapes are the smallest that reach every allocation site: B = 37 (a multiple of nothing) then B = 130 (every
batch-sized buffer is dropped and grown), L-A staging (regular, irregular: the row pointers; bf16: the rounded
copies), the backward's state, both parameter layouts of set_precision, the optimiser's slots / grouping scratch
/ gradient buffers, a table's line copy, a two-rank in-process shard group."""
import contextlib
import gc

import numpy as np
import pytest

import rmx
import lifecycle_common as lc
from lifecycle_common import F, K, V

pytestmark = pytest.mark.gpu

MODELS = [(k, False) for k in lc.FP32_KINDS] + [("dcn", True), ("pnn", True)]
MODEL_IDS = ["%s%s" % (k, "_bf16" if b else "") for k, b in MODELS]
BS = (37, 130)


@pytest.fixture(scope="module")
def ctx():
    c = rmx.default_context()
    lc.table(c), lc.table(c, True)  # the shared tables outlive this file: made before any first reading
    return c


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    lc.restore_knobs()
    rmx.set_tuning("table_lines", None)


@contextlib.contextmanager
def balanced():
    """Yields a function the body calls while its objects live; checks the two counters around the body."""
    gc.collect()  # what earlier tests left for the collector goes now, not between the two readings
    before = rmx.debug_live_device_memory()
    seen = []
    yield lambda: seen.append(rmx.debug_live_device_memory())
    gc.collect()
    after = rmx.debug_live_device_memory()
    assert seen, "the test took no reading while its objects lived"
    for b, n in seen:
        assert b > before[0] and n > before[1], ("while alive", (b, n), "before", before)
    assert after == before, ("(bytes, buffers) after", after, "before", before)


def _forward_ids(ctx, m, B, bf16=False):
    out = rmx.DeviceArray(ctx, B, np.float32)
    m.forward_ids(lc.table(ctx, bf16), B, lc.dev_ids(ctx, B), out)
    ctx.sync()


def _forward_la(m, kind, B, bf16=False, index=None):
    w, e = lc.host_rows(B, 0, bf16)
    index = lc.regular_index(B) if index is None else index
    feats = lc.host_ids(B).reshape(-1).astype(np.int64)
    bias = np.array([lc.BIAS], np.float32)
    if kind == "lr":
        return m.forward(B, (index, feats), bias, w)
    return m.forward(B, (index, feats), bias, w, e, K, lc.host_mats(kind, bf16), m.getMatsSize())


@pytest.mark.parametrize("kind,bf16", MODELS, ids=MODEL_IDS)
def test_model_forward(ctx, kind, bf16):
    """forward_ids at B = 37 then 130 (the regrow), then the L-A forward at B = 37."""
    with balanced() as reading:
        m = lc.new_model(kind, bf16)
        for B in BS:
            _forward_ids(ctx, m, B, bf16)
        _forward_la(m, kind, BS[0], bf16)
        reading()
        m.close()


def test_la_irregular_index(ctx):
    """An index that is no n / F (here: the rows in descending order): the CSR first order and its row pointers."""
    with balanced() as reading:
        m = lc.new_model("deepfm")
        _forward_la(m, "deepfm", BS[0], index=lc.regular_index(BS[0])[::-1].copy())
        reading()
        m.close()


@pytest.mark.parametrize("kind", lc.FP32_KINDS)
def test_model_backward(ctx, kind):
    with balanced() as reading:
        m = lc.new_model(kind)
        lc.backward_once(ctx, kind, BS[0], m=m)
        reading()
        m.close()


def test_la_backward(ctx):
    """rmx_backward's own staging (the gradient arrays it copies back)."""
    B = BS[0]
    with balanced() as reading:
        m = lc.new_model("deepfm")
        w, e = lc.host_rows(B)
        index, feats = lc.regular_index(B), lc.host_ids(B).reshape(-1).astype(np.int64)
        m.backward(B, (index, feats), np.array([lc.BIAS], np.float32), w.copy(), e.copy(), K,
                   lc.host_mats("deepfm").copy(), m.getMatsSize(), lc.host_targets(B))
        reading()
        m.close()


def test_set_precision_round_trip(ctx):
    """PNN fp32 -> bf16 -> fp32: each switch drops one parameter layout and the [x | ip] rows, and builds the other."""
    with balanced() as reading:
        m = lc.new_model("pnn")
        _forward_ids(ctx, m, BS[0])
        for bf16 in (True, False):
            m.setPrecision(rmx.DTYPE_BF16 if bf16 else rmx.DTYPE_F32)
            m.setMats(lc.host_mats("pnn", bf16))
            _forward_ids(ctx, m, BS[0], bf16)
            reading()
        m.close()


def test_optimizer_train_steps(ctx):
    """Adam (two state slots) and train_step_ids at B = 37 then 130; on a table of its own, which the steps update."""
    with balanced() as reading:
        t = rmx.EmbeddingTable(ctx, V, K)
        t.fill_synthetic(lc.SEED_TAB)
        m = lc.new_model("deepfm")
        opt = rmx.Optimizer(m, t, "adam", eta=0.01)
        for B in BS:
            targets = rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(lc.host_targets(B)))
            m.train_step_ids(t, opt, B, lc.dev_ids(ctx, B), targets)
        reading()
        opt.close()
        m.close()
        t.close()


def test_table_with_line_copy(ctx):
    with balanced() as reading:
        rmx.set_tuning("table_lines", 1)
        b0, n0 = rmx.debug_live_device_memory()
        t = rmx.EmbeddingTable(ctx, V, K)
        t.fill_synthetic(lc.SEED_TAB)
        b1, n1 = rmx.debug_live_device_memory()
        reading()
        t.close()
    assert (b1 - b0, n1 - n0) == (4 * V * (1 + K + 32), 3)  # w [V], emb [V][k] and the [V][32] line copy


def test_shard_group(ctx):
    """Two in-process ranks: one pull and its forward each."""
    import threading
    N, B = 2, BS[0]
    errs = []
    with balanced() as reading:
        g = rmx.ExchangeGroup(N)
        gate = threading.Barrier(N)

        def rank(r):
            try:
                c = rmx.Context(0)
                sh = rmx.ShardedTable(c, V, K, N, r, group=g)
                sh.fill_synthetic(lc.SEED_TAB)
                m = lc.new_model("deepfm")
                ids = rmx.DeviceArray.from_numpy(c, np.ascontiguousarray(lc.host_ids(B, r * B)))
                out = rmx.DeviceArray(c, B, np.float32)
                sh.pull(ids, B * F, 0, c.stream)
                m.forward_pulled(sh, B, 0, out, c.stream)
                c.sync()
                gate.wait(60)  # both ranks alive at the reading
                if r == 0:
                    reading()
                gate.wait(60)
                sh.close()
                m.close()
            except BaseException as e:  # noqa: BLE001 -- reported below with the rank
                gate.abort()
                errs.append((r, e))

        ts = [threading.Thread(target=rank, args=(r,)) for r in range(N)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts), "a rank hung"
        assert not errs, "rank %d failed: %r" % errs[0]
        g.close()
