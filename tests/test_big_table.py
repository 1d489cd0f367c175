"""Every table path past 2^31 elements and 4 GiB offsets (big_table.py): tables of 4.3 to 17.3 GB whose rows are
read and written around the rows where an offset crosses 2^31 / 2^32 elements or 2^32 / 2^33 / 2^34 bytes.

Two references.  The anchor: rmx_gather of the whole id pool equals the host generator bit for bit, and forward_ids
at B <= 300 is within the sweep's bars (1e-5 of the f64 oracle; 2e-4 of the bf16 emulation) on rows the host
generated.  Address invariance: the same model on the same batch, once on the big table and once on the compact
twin (row r = pool[r]'s row, uploaded from the host generator; ids = ranks), gives the same stage list and the same
bits -- forward_ids, encoder_ids, predict_ids, every output of backward_ids, the optimiser's rows and state.  No
stage list here depends on V (the dispatch reads B, F, k, the widths and the knobs), so no case falls back to the
oracle.  Writes are checked twice: the touched rows, and the rows a truncated offset would have hit -- every pool
row not touched (the pool holds the aliases of its own rows under each truncation model) with its neighbours, and
64 random windows of 4,096 rows -- which must still hold the generator's bits.

One big table is alive at a time: one test class per table / dtype / line copy with a class-scoped `big` fixture,
whose teardown asserts that the library's live device memory is back at the reading before it, and every test asserts
the 40 GiB cap.  A test skips only when the big table cannot be allocated (RMX_E_NOMEM).
test_big_table_cpu.py holds what makes a failure here the kernels'."""
import ctypes

import numpy as np
import pytest

import big_table as bt
import optim_ref as R
import shard_ref
import oracle_ctypes as oc
import rmx
import shape_cases as sc
from rmx import _lib

pytestmark = pytest.mark.gpu

NAN = 0x7FC07FC0
# the paths of big_table.OTHER_PATHS: (a class that runs it, its test) -- test_big_table_cpu.py holds each to exist
PATH_TESTS = {
    "rmx_gather": ("Test_T16_fp32", "test_gather_of_the_pool_is_the_generator"),
    "rmx_gather bf16": ("Test_T16_bf16", "test_gather_of_the_pool_is_the_generator"),
    "fill_synthetic / pack_lines": ("Test_T16_fp32_lines", "test_gather_of_the_pool_is_the_generator"),
    "param_io put / get rows": ("Test_T10_fp32", "test_param_io_across_the_boundaries"),
    "param_io put rows into lines": ("Test_T16_fp32_lines", "test_param_io_across_the_boundaries"),
    "optim apply (tab_update)": ("Test_T16_fp32", "test_optimiser_steps"),
    "optim state put / get rows": ("Test_T10_fp32", "test_optimiser_steps"),
    "train_step_ids": ("Test_T16_fp32_lines", "test_optimiser_steps"),
    "shard gather": ("Test_shard_N1_default", "test_shard_gather_and_rows"),
    "shard forward / pull": ("Test_shard_N2_default", "test_shard_forward_and_backward"),
    "shard put / get rows": ("Test_shard_N1_key0", "test_shard_gather_and_rows"),
    "shard push (train_step_sharded)": ("Test_shard_N2_key0", "test_shard_train_steps"),
}
WORST = {"fp32": 0.0, "bf16": 0.0}  # the worst oracle errors of the anchors (printed by the last test)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return np.asarray(a).size == np.asarray(b).size and np.array_equal(_bits(a), _bits(b))


def live():
    return rmx.debug_live_device_memory()[0]


def under_cap():
    """A sampled bound: the library offers a live reading, no peak, so it is read after every large allocation (a
    table, an optimiser's state) and at the end of every test; what a call holds only while it runs is not seen."""
    n = live()
    assert n <= bt.MEM_CAP, "live device memory %.1f GiB is over the 40 GiB cap" % (n / 2 ** 30)
    return n


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63  # hip_runtime_api.h hipDeviceAttribute_t (ROCm 6 / 7)


@pytest.fixture(scope="module")
def ncu(ctx):
    """The device's CU count: the split GEMM and the CIN choose their tiles by it (test_batch_sweep.py's)."""
    hip = ctypes.CDLL("libamdhip64.so")
    d, n = ctypes.c_int(0), ctypes.c_int(0)
    assert hip.hipGetDevice(ctypes.byref(d)) == 0
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, d) == 0
    assert 0 < n.value <= 4096
    return n.value


def check_claims(case, ncu, bf16=False):
    """What the case claims of (row, batch) holds on this device's CU count too: where it does not, the kernel the
    case is named for is not the one that runs, and the case fails rather than pass on another path."""
    for claim in case.claims:
        assert bt.holds(claim, bt.case(case.row), case.B, ncu, bf16), "%s: %s at B = %d does not reach %s on %d CUs" % (
            case.path, case.row, case.B, claim, ncu)


def check_stages(case, stages):
    for s in case.want:
        assert s in stages, (case.path, "stage missing", s, stages)
    for s in case.absent:
        assert s not in stages, (case.path, "stage not expected", s, stages)


class Big:
    """One big table (fill_synthetic), its id pool and its compact twin; a line-copy table also has a twin
    without the copy."""

    def __init__(self, ctx, name, bf16, lines):
        self.ctx, self.t, self.bf16, self.lines = ctx, bt.TABLES[name], bf16, lines
        self.p = bt.pool_of(self.t, bf16, lines)
        self.dtype = rmx.DTYPE_BF16 if bf16 else rmx.DTYPE_F32
        self.table = self.twin = self.twin_dense = None
        t = self.t
        rmx.set_tuning("table_lines", lines)
        try:
            self.table = rmx.EmbeddingTable(ctx, t.V, t.k, self.dtype)
            self.table.fill_synthetic(bt.SEED_TAB)
        except rmx.RmxError as e:
            self.close()
            if e.args and e.args[0] == _lib.RMX_E_NOMEM:
                pytest.skip("RMX_E_NOMEM: no room for %s (%s)" % (name, e))
            raise
        under_cap()
        self.w, self.e = bt.rows_of(t, self.p.ids)  # fp32, never rounded: a bf16 table rounds an upload itself
        self.twin = self._twin()
        if lines:
            rmx.set_tuning("table_lines", 0)
            self.twin_dense = self._twin()
            rmx.set_tuning("table_lines", lines)

    def _twin(self):
        tw = rmx.EmbeddingTable(self.ctx, len(self.p.ids), self.t.k, self.dtype)
        tw.upload(self.w, self.e)
        return tw

    def rows(self, ids):
        """The generator's rows of ids as the table stores them."""
        return bt.rows_of(self.t, ids, self.bf16)

    def close(self):
        for o in (self.twin_dense, self.twin, self.table):
            if o is not None:
                o.close()
        rmx.set_tuning("table_lines", None)


def held(ctx, make, what):
    """A class-scoped fixture's body: the object while the class runs; afterwards the library's live device memory
    is back at the reading before it."""
    ctx.sync()
    start = rmx.debug_live_device_memory()
    b = make()
    yield b
    b.close()
    ctx.sync()
    assert rmx.debug_live_device_memory() == start, "device memory held after %s was closed" % what


def cfg_id(c):
    return "%s-%s%s" % (c[0], "bf16" if c[1] else "fp32", "-lines" if c[2] else "")


ALL_CFG = bt.configs()
F32_CFG = [c for c in ALL_CFG if not c[1]]


def cases_of(cfg, cases, key=lambda c: (c.table, c.bf16, c.lines)):
    """pytest params of the cases of one big table."""
    return [pytest.param(c, id="%s-%s-B%d-%d" % (c.path.replace(" ", "_").replace("/", ""), c.row, c.B, i))
            for i, c in enumerate(cases) if key(c) == cfg]


class Knobs:
    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs:
            rmx.set_tuning(k, v)

    def __exit__(self, *a):
        for k, _ in self.knobs:
            rmx.set_tuning(k, None)


def dev(ctx, a):
    return rmx.DeviceArray.from_numpy(ctx, np.ascontiguousarray(a))


def run_reads(ctx, m, table, B, ids_d):
    """(stage list, {entry point: output}) of forward_ids, encoder_ids and predict_ids (in chunks of 4,096)."""
    out = rmx.DeviceArray(ctx, B, np.float32)
    res = {}
    m.set_timing(True)
    m.forward_ids(table, B, ids_d, out)
    ctx.sync()
    stages = sorted(m.get_timing()[0])
    m.set_timing(False)
    res["forward_ids"] = out.numpy().copy()
    out.upload(np.full(B, np.nan, np.float32))
    m.encoder_ids(table, B, ids_d, out)
    ctx.sync()
    res["encoder_ids"] = out.numpy().copy()
    out.upload(np.full(B, np.nan, np.float32))
    m.predict_ids(table, B, ids_d, out, batch=min(B, 4096))
    ctx.sync()
    res["predict_ids"] = out.numpy().copy()
    out.free()
    return stages, res


# ---- reads: the anchor ---------------------------------------------------------------------------------------
def gather_of_the_pool_is_the_generator(ctx, big):
    """rmx_gather (gather_kernel) of every pool id, in pool order and shuffled: the generator's bits."""
    p, k = big.p, big.t.k
    w_ref, e_ref = big.rows(p.ids)
    for order in (np.arange(len(p.ids)), np.random.default_rng(1).permutation(len(p.ids))):
        ids_d = dev(ctx, p.ids[order].astype(np.int32))
        w_d, e_d = rmx.DeviceArray(ctx, len(order), np.float32), rmx.DeviceArray(ctx, len(order) * k, np.float32)
        big.table.gather(ids_d, len(order), w_d, e_d)
        ctx.sync()
        assert same_bits(w_d.numpy(), w_ref[order]), "first-order weights"
        assert same_bits(e_d.numpy(), e_ref[order]), "embedding rows"
        for a in (ids_d, w_d, e_d):
            a.free()
    tw, te = big.twin.download()
    assert same_bits(tw, w_ref) and same_bits(te, e_ref)  # the twin holds the pool's rows
    under_cap()


# ---- reads: every forward path -------------------------------------------------------------------------------
def read_paths(ctx, ncu, big, case):
    c = bt.case(case.row)
    p, t, B = big.p, big.t, case.B
    check_claims(case, ncu, case.bf16)
    ids = bt.batch_ids(p, B, c.F, 0xB16 + B)
    assert bt.keeps_rule(p, ids)
    ids_d, tw_d = dev(ctx, ids.reshape(-1)), dev(ctx, bt.rank(p, ids).reshape(-1))
    m_big = bt.rmx_model(case.row, t.V, case.bf16, case.cin16)
    m_tw = bt.rmx_model(case.row, len(p.ids), case.bf16, case.cin16)
    try:
        with Knobs(case.knobs):
            st_big, got = run_reads(ctx, m_big, big.table, B, ids_d)
            st_tw, ref = run_reads(ctx, m_tw, big.twin, B, tw_d)
            dense = run_reads(ctx, m_tw, big.twin_dense, B, tw_d)[1] if big.lines else None
        print("%s: %s on %s B=%d: stages %s" % (case.path, case.row, cfg_id((case.table, case.bf16, case.lines)), B,
                                                 st_big))
        assert st_big == st_tw, (st_big, st_tw)
        check_stages(case, st_big)
        if case.path.startswith("tail_fo"):  # the tail's head sums the first order: no kernel of its own
            assert "first_order" not in st_big, st_big
        for what in got:
            assert np.isfinite(got[what]).all(), what
            assert same_bits(got[what], ref[what]), "%s: big table and twin differ, max |d| %.3g" % (
                what, np.abs(got[what] - ref[what]).max())
            if dense is not None:  # the line copy holds the rows' bits: the project's equality (test_head_s3.py,
                # test_encoder_v2.py, test_device_memory.py) is bit for bit
                assert same_bits(got[what], dense[what]), "%s: line copy and dense rows differ" % what
        if B <= 300:  # the anchor: rows from the host generator through the oracle
            w, e = big.rows(ids.reshape(-1))
            if case.cin16:
                pass  # (the bf16 CIN's bar is test_cin_bf16.py's own; here the twin carries the check)
            else:
                orc = bt.oracle_rows(case.row, w, e.ravel(), 2 if case.bf16 else 1, case.bf16)
                err = float(np.abs(got["forward_ids"] - orc).max())
                kind = "bf16" if case.bf16 else "fp32"
                WORST[kind] = max(WORST[kind], err)
                print("  max |p - p_oracle| = %.3g (%s)" % (err, kind))
                assert err <= (sc.TOL_BF16 if case.bf16 else sc.TOL), (case.row, err)
    finally:
        for o in (ids_d, tw_d, m_big, m_tw):
            o.close()
    under_cap()


# ---- backward ------------------------------------------------------------------------------------------------
class Backward:
    """backward_ids on fixed ids / targets; the five outputs are NaN before every call."""

    def __init__(self, ctx, c, B, k, ml):
        self.ctx, self.B = ctx, B
        self.targets = dev(ctx, sc.host_targets(B))
        sizes = (1, B * c.F, B * c.F * k, max(ml, 1), 1)
        self.ml = ml
        self.outs = [rmx.DeviceArray(ctx, n, np.float32) for n in sizes]
        self.nans = [np.full(n, np.nan, np.float32) for n in sizes]
        self.written = (True, c.kind != "dnn", c.kind != "lr", c.kind != "lr", True)

    def run(self, m, table, ids_d):
        for o, n in zip(self.outs, self.nans):
            o.upload(n)
        g = self.outs
        m.set_timing(True)
        m.backward_ids(table, self.B, ids_d, self.targets, g[0], g[1], g[2], g[3] if self.ml else None, g[4])
        self.ctx.sync()
        stages = sorted(m.get_timing()[0])
        m.set_timing(False)
        return stages, [o.numpy().copy() for o in self.outs]

    def close(self):
        for o in self.outs + [self.targets]:
            o.free()


BWD_KEY = lambda c: (c.table, False, 0)


def backward_paths(ctx, ncu, big, case):
    c = bt.case(case.row)
    p, t, B = big.p, big.t, case.B
    check_claims(case, ncu)
    ids = bt.batch_ids(p, B, c.F, 0xBAC + B)
    ids_d, tw_d = dev(ctx, ids.reshape(-1)), dev(ctx, bt.rank(p, ids).reshape(-1))
    m_big, m_tw = bt.rmx_model(case.row, t.V), bt.rmx_model(case.row, len(p.ids))
    bw = Backward(ctx, c, B, c.k, len(bt.host_mats(case.row)))
    try:
        with Knobs(case.knobs):
            st_big, got = bw.run(m_big, big.table, ids_d)
            st_tw, ref = bw.run(m_tw, big.twin, tw_d)
        print("%s: %s on %s B=%d: loss %.6g, stages %s" % (case.path, case.row, case.table, B, got[4][0], st_big))
        assert st_big == st_tw, (st_big, st_tw)
        check_stages(case, st_big)
        for i, (g, r, wr) in enumerate(zip(got, ref, bw.written)):
            if wr:
                assert np.isfinite(g).all(), i
            assert same_bits(g, r), "backward output %d: big table and twin differ" % i
        assert np.isfinite(got[4][0]) and got[4][0] > 0
        if c.kind != "dnn":
            assert np.any(got[1] != 0)
    finally:
        for o in (ids_d, tw_d, m_big, m_tw, bw):
            o.close()
    under_cap()


# ---- leftovers -----------------------------------------------------------------------------------------------
LEFT = {"T16": "deepfm_f13k16_401x37", "T32": "dnn_f3k32_520", "T8": "dnn_f17k8_500x7", "T10": "deepfm_f7k10_33x20",
        "T1": "deepfm_f2k1_5x3"}


def nan_leftovers(ctx, big):
    """One forward and one backward per table with the model's scratch and every CU's LDS full of NaNs: the bits of
    the zero-filled run (the model is primed at a larger batch first, so the scratch is larger than the call's)."""
    row = LEFT[big.t.name]
    c, p, B = bt.case(row), big.p, 300
    m = bt.rmx_model(row, big.t.V)
    prime = dev(ctx, bt.batch_ids(p, 2049, c.F, 3).reshape(-1))
    ids_d = dev(ctx, bt.batch_ids(p, B, c.F, 4).reshape(-1))
    out = rmx.DeviceArray(ctx, 2049, np.float32)
    bw0, bw = Backward(ctx, c, 2049, c.k, len(bt.host_mats(row))), Backward(ctx, c, B, c.k, len(bt.host_mats(row)))
    try:
        m.forward_ids(big.table, 2049, prime, out)
        bw0.run(m, big.table, prime)
        kept = None
        for pat in (0, NAN):
            assert rmx.debug_poison_workspace(m, pat) > 0
            rmx.debug_fill_lds(ctx, pat)
            m.forward_ids(big.table, B, ids_d, out)
            ctx.sync()
            fwd = out.numpy()[:B].copy()
            assert rmx.debug_poison_workspace(m, pat) > 0
            rmx.debug_fill_lds(ctx, pat)
            got = [fwd] + bw.run(m, big.table, ids_d)[1]
            if kept is None:
                kept = got
                assert np.isfinite(fwd).all()
            for i, (g, r) in enumerate(zip(got, kept)):
                assert same_bits(g, r), "%s output %d, pattern %s" % (row, i, hex(pat))
    finally:
        for o in (prime, ids_d, out, bw0, bw, m):
            o.close()
    under_cap()


# ---- writes --------------------------------------------------------------------------------------------------
def alias_spans(ids, k, forms, V):
    """[(first row, end)]: the rows that hold the truncated address of the first or last element of any of `ids`
    under any truncation model, in any of the forms, each with its two neighbours."""
    ids = np.unique(np.asarray(ids, np.int64))
    al = [bt.alias_rows(ids, k, f) for f in forms]
    al = np.unique(np.concatenate(al)) if al else np.zeros(0, np.int64)
    return [(max(a - 1, 0), min(a + n + 1, V)) for a, n in bt.runs(al)]


def check_untouched(big, touched, what, state=None):
    """The places a truncated write would land: the alias windows (+- 1 row) of every touched id in every form the
    table or the state is held in, every pool row with its two neighbours, and 64 random windows of 4,096 rows.
    Outside `touched` they still hold the generator's bits (state: an optimiser's slots hold zeros)."""
    t, rng = big.t, np.random.default_rng(len(touched))
    touched = np.unique(np.asarray(touched, np.int64))
    spans = alias_spans(touched, t.k, bt.forms_of(t, big.bf16, big.lines), t.V)
    assert spans or not len(touched) or touched.max() < big.p.bounds[0]
    spans += [(max(i0 - 1, 0), min(i0 + n + 1, t.V)) for i0, n in bt.runs(big.p.ids)]
    spans += [(int(r), int(r) + 4096) for r in rng.integers(0, t.V - 4096, 64)]
    for a, b in spans:
        ids = np.arange(a, b)
        keep = ~np.isin(ids, touched)
        w, e = big.table.download_rows(a, b - a)
        w_ref, e_ref = big.rows(ids)
        assert same_bits(w[keep], w_ref[keep]), "%s: first-order weights changed in rows [%d, %d)" % (what, a, b)
        assert same_bits(e[keep], e_ref[keep]), "%s: embedding rows changed in rows [%d, %d)" % (what, a, b)
        for opt, slots in (state or ()):
            for slot in range(slots):
                sw, se, _ = opt.state_download_rows(slot, a, b - a)
                assert not sw[keep].any() and not se[keep].any(), "%s: state slot %d written in [%d, %d)" % (
                    what, slot, a, b)


def restore(big, ranges):
    for a, n in ranges:
        w, e = bt.rows_of(big.t, np.arange(a, a + n))
        big.table.upload_rows(a, w, e)


def param_io_across_the_boundaries(ctx, big, layout, chunk):
    """upload_rows / download_rows over [b - 1000, b + 1000) for every boundary b and over [V - 1000, V): the round
    trip returns the uploaded bits (a bf16 table: rounded), nothing else moves, and with a line copy a DeepFM
    forward reads the new rows from it."""
    t, p = big.t, big.p
    ranges = [(b - 1000, 2000) for b in p.bounds] + [(t.V - 1000, 1000)]
    rng = np.random.default_rng(17)
    rmx.set_tuning("io_chunk_rows", chunk)
    try:
        new = {}
        for a, n in ranges:
            w = rng.uniform(-0.05, 0.05, n).astype(np.float32)
            e = rng.uniform(-0.05, 0.05, (n, t.k)).astype(np.float32)
            new[a] = (w, e)
            big.table.upload_rows(a, w, np.ascontiguousarray(e.T) if layout == rmx.LAYOUT_K_MAJOR else e, layout)
        for a, n in ranges:
            w, e = new[a]
            if big.bf16:
                w, e = oc.round_bf16(w), oc.round_bf16(e).reshape(n, t.k)
            gw, ge = big.table.download_rows(a, n, layout)
            assert same_bits(gw, w), (a, "weights")
            assert same_bits(ge.T if layout == rmx.LAYOUT_K_MAJOR else ge, e), (a, "embedding")
        touched = np.concatenate([np.arange(a, a + n) for a, n in ranges])
        rmx.set_tuning("io_chunk_rows", None)
        check_untouched(big, touched, "upload_rows")
        if t.k == 16:  # a forward over the new rows (with a line copy: it got them too)
            row = "deepfm_f13k16_209x37"
            c, B = bt.case(row), 300
            ids = touched[rng.integers(0, len(touched), (B, c.F))]
            ids[:, 0] = p.ids[rng.integers(0, 64, B)]
            m = bt.rmx_model(row, t.V, big.bf16)
            ids_d, out = dev(ctx, ids.astype(np.int32).reshape(-1)), rmx.DeviceArray(ctx, B, np.float32)
            m.forward_ids(big.table, B, ids_d, out)
            ctx.sync()
            w_all = np.concatenate([new[a][0] for a, _ in ranges])
            e_all = np.concatenate([new[a][1] for a, _ in ranges])
            pos = np.searchsorted(touched, ids.reshape(-1))
            hit = touched[np.minimum(pos, len(touched) - 1)] == ids.reshape(-1)
            w0, e0 = bt.rows_of(t, ids.reshape(-1))
            w_in = np.where(hit, w_all[np.minimum(pos, len(touched) - 1)], w0)
            e_in = np.where(hit[:, None], e_all[np.minimum(pos, len(touched) - 1)], e0)
            if big.bf16:
                w_in, e_in = oc.round_bf16(w_in), oc.round_bf16(e_in)
            orc = bt.oracle_rows(row, w_in, e_in.ravel(), 2 if big.bf16 else 1, big.bf16)
            err = float(np.abs(out.numpy() - orc).max())
            print("forward over the uploaded rows: max |p - p_oracle| = %.3g" % err)
            assert err <= (sc.TOL_BF16 if big.bf16 else sc.TOL)
            for o in (ids_d, out, m):
                o.close()
    finally:
        restore(big, ranges)
        rmx.set_tuning("io_chunk_rows", None)
    w, e = big.table.download_rows(ranges[-1][0], ranges[-1][1])
    assert same_bits(e, big.rows(np.arange(t.V - 1000, t.V))[1])
    under_cap()


# ---- the optimiser -------------------------------------------------------------------------------------------
OPT_ROWS = {"T16": "deepfm_f13k16_209x37", "T10": "deepfm_f7k10_33x20"}
# (Adam's two slots beside T16's line copy: 44 GB, over the cap)
OPT_KINDS = {("T10", False, 0): ("sgd", "adam"), ("T16", False, 0): ("sgd", "adam"), ("T16", False, 1): ("sgd",)}
BAD_IDS = (-1, np.iinfo(np.int32).max)


def pool_rows(obj, p, slot=None):
    """(w, e) of every pool row through download_rows (slot: an optimiser's state)."""
    ws, es = [], []
    for a, n in bt.runs(p.ids):
        r = obj.download_rows(a, n) if slot is None else obj.state_download_rows(slot, a, n)
        ws.append(r[0])
        es.append(r[1])
    return np.concatenate(ws), np.concatenate(es)


def twin_rows(obj, n, slot=None):
    r = obj.download_rows(0, n) if slot is None else obj.state_download_rows(slot, 0, n)
    return r[0], r[1]


def optimiser_steps(ctx, big, kind):
    """Three apply steps on synthetic gradients, then three train_step_ids, with duplicate pool ids and ids outside
    the table (V + 12345, -1, int32 max: skipped): rows and both state slots against optim_ref on the pool rows
    (SGD: bit for bit; Adam: test_optim.py's 1e-5 of the step), bit for bit against the same steps on the twin,
    nothing written anywhere else; with a line copy, the forward after the steps reads the stepped rows."""
    t, p = big.t, big.p
    row = OPT_ROWS[t.name]
    c, B, n = bt.case(row), 64, len(p.ids)
    hp = dict(eta=1.0) if kind == "sgd" else dict(eta=0.05)
    m_big, m_tw = bt.rmx_model(row, t.V), bt.rmx_model(row, n)
    ml = len(bt.host_mats(row))
    o_big = o_tw = None
    touched = set()
    try:
        o_big, o_tw = rmx.Optimizer(m_big, big.table, kind, **hp), rmx.Optimizer(m_tw, big.twin, kind, **hp)
        under_cap()
        ref = R.RefOptim(kind, R.hyper(kind, **hp), big.w, big.e, bt.host_mats(row), np.float32(sc.BIAS),
                         np.float32 if kind == "sgd" else np.float64)
        rng = np.random.default_rng(99)
        for step in range(3):
            ids = bt.batch_ids(p, B, c.F, 40 + step).reshape(-1)
            ids[5::97] = ids[5]  # one id many times
            bad = rng.choice(len(ids), 6, replace=False)
            ids_tw = bt.rank(p, ids)
            ids[bad] = [t.V + 12345, -1, np.iinfo(np.int32).max] * 2
            ids_tw[bad] = [n + 12345, -1, np.iinfo(np.int32).max] * 2
            touched |= set(ids[(ids >= 0) & (ids < t.V)].tolist())
            g = dict(g_bias=rng.normal(0, 1, 1), g_w=rng.normal(0, 1, len(ids)), g_emb=rng.normal(0, 1, (len(ids), t.k)),
                     g_mats=rng.normal(0, 1, ml))
            g = {k_: v.astype(np.float32) for k_, v in g.items()}
            prev = (ref.w.copy(), ref.emb.copy())
            ref.apply(ids_tw.astype(np.int64), g["g_bias"], g["g_w"], g["g_emb"], g["g_mats"])
            for opt, h in ((o_big, ids), (o_tw, ids_tw)):
                arrs = [dev(ctx, h)] + [dev(ctx, g[k_]) for k_ in ("g_bias", "g_w", "g_emb", "g_mats")]
                opt.apply(B, *arrs)
                ctx.sync()
                for a in arrs:
                    a.free()
            check_step(big, o_big, o_tw, m_big, m_tw, ref, prev, kind, "apply %d" % (step + 1))
        for step in range(3):  # the whole training step: the backward reads the rows the apply then writes
            ids = bt.batch_ids(p, B, c.F, 50 + step)
            touched |= set(ids.reshape(-1).tolist())
            tg = dev(ctx, sc.host_targets(B))
            a, b = dev(ctx, ids.reshape(-1)), dev(ctx, bt.rank(p, ids).reshape(-1))
            la = m_big.train_step_ids(big.table, o_big, B, a, tg)
            lb = m_tw.train_step_ids(big.twin, o_tw, B, b, tg)
            assert np.float32(la) == np.float32(lb) and np.isfinite(la), step
            check_step(big, o_big, o_tw, m_big, m_tw, None, None, kind, "train step %d" % (step + 1))
            for o in (a, b, tg):
                o.free()
        assert o_big.steps == o_tw.steps == 6
        check_untouched(big, sorted(touched), "optimiser", [(o_big, R.NSLOTS[kind])])
        if R.NSLOTS[kind]:  # state rows across the boundaries: an upload comes back, and lands nowhere else
            st = np.concatenate([np.arange(b0 - 1000, b0 + 1000) for b0 in p.bounds])
            spans = alias_spans(st, t.k, ("f32",), t.V)  # (the state is dense fp32 [V][k] and [V])
            assert spans
            before = [o_big.state_download_rows(1, a_, b_ - a_)[:2] for a_, b_ in spans]
            for b0 in p.bounds:
                w = rng.uniform(-1, 1, 2000).astype(np.float32)
                e = rng.uniform(-1, 1, (2000, t.k)).astype(np.float32)
                assert o_big.state_upload_rows(1, b0 - 1000, w, e) == 2000
                gw, ge, owned = o_big.state_download_rows(1, b0 - 1000, 2000)
                assert same_bits(gw, w) and same_bits(ge, e) and owned.all()
                z = np.zeros_like(e)
                o_big.state_upload_rows(0, b0 - 1000, w * 0, z)  # (slot 0 of the range: zeros, for the check below)
            for (a_, b_), (w0, e0) in zip(spans, before):  # slot 1 where a truncated upload would have landed
                keep = ~np.isin(np.arange(a_, b_), st)
                w1, e1, _ = o_big.state_download_rows(1, a_, b_ - a_)
                assert same_bits(w1[keep], w0[keep]) and same_bits(e1[keep], e0[keep]), (
                    "state slot 1 moved in rows [%d, %d) under an upload elsewhere" % (a_, b_))
            s1, t1 = pool_rows(o_big, p, 1), twin_rows(o_tw, n, 1)
            keep = ~np.isin(p.ids, st)
            assert same_bits(s1[0][keep], t1[0][keep]) and same_bits(s1[1][keep], t1[1][keep])
            s0 = pool_rows(o_big, p, 0)
            keep = ~np.isin(p.ids, st)
            t0 = twin_rows(o_tw, n, 0)
            assert same_bits(s0[1][keep], t0[1][keep]), "state slot 0 moved under an upload into slot 1"
        if big.lines:  # the forward reads the line copy: it must hold the stepped rows
            ids = bt.batch_ids(p, 300, c.F, 77)
            a, b = dev(ctx, ids.reshape(-1)), dev(ctx, bt.rank(p, ids).reshape(-1))
            got = run_reads(ctx, m_big, big.table, 300, a)[1]["forward_ids"]
            for tw in (big.twin, big.twin_dense):
                if tw is big.twin_dense:  # the dense twin takes the stepped rows from the stepped twin
                    w, e = big.twin.download()
                    tw.upload(w, e)
                assert same_bits(got, run_reads(ctx, m_tw, tw, 300, b)[1]["forward_ids"])
            a.free()
            b.free()
    finally:
        for o in (o_big, o_tw):
            if o is not None:
                o.close()
        m_big.close()
        m_tw.close()
        restore(big, bt.runs(np.array(sorted(touched), np.int64)) if touched else [])
        big.twin.upload(big.w, big.e)
        if big.twin_dense is not None:
            rmx.set_tuning("table_lines", 0)
            big.twin_dense.upload(big.w, big.e)
            rmx.set_tuning("table_lines", big.lines)
    check_untouched(big, [], "restore")
    under_cap()


def check_step(big, o_big, o_tw, m_big, m_tw, ref, prev, kind, what):
    p, n = big.p, len(big.p.ids)
    gw, ge = pool_rows(big.table, p)
    tw, te = twin_rows(big.twin, n)
    assert same_bits(gw, tw) and same_bits(ge, te), what + ": rows of the big table and the twin differ"
    assert same_bits(m_big.getMats(), m_tw.getMats()) and np.float32(m_big.getBias()) == np.float32(m_tw.getBias()), what
    for slot in range(R.NSLOTS[kind]):
        sw, se = pool_rows(o_big, p, slot)
        uw, ue = twin_rows(o_tw, n, slot)
        assert same_bits(sw, uw) and same_bits(se, ue), "%s: state slot %d differs from the twin's" % (what, slot)
        if ref is not None:
            for got, r in ((sw, ref.s_w[slot]), (se, ref.s_emb[slot])):
                err = np.abs(got.reshape(-1) - r.reshape(-1)).max() / np.abs(r).max()
                assert err <= 1e-5, (what, slot, err)
    if ref is None:
        return
    if kind == "sgd":
        assert same_bits(gw, ref.w) and same_bits(ge, ref.emb), what + ": rows differ from optim_ref"
        assert same_bits(m_big.getMats(), ref.mats)
    else:
        for got, r, r0 in ((gw, ref.w, prev[0]), (ge, ref.emb, prev[1])):
            d_ref = r - r0
            d_got = got.astype(np.float64).reshape(r.shape) - r0
            err = np.abs(d_got - d_ref).max() / np.abs(d_ref).max()
            print("%s %s: step error %.3g of the largest step" % (what, kind, err))
            assert err <= 1e-5, (what, err)


# ---- shards --------------------------------------------------------------------------------------------------
SHARD_V, SHARD_K = bt.TABLES["T16"].V, 16
SHARDS = [(1, "default"), (1, "key0"), (2, "default"), (2, "key0")]
SHARD_FORMS = ("lines_f32", "f32")  # a partition's [rows][32] lines; the optimiser's state [rows][16] (and [rows])


def shard_pool(N, key):
    """(ids, their owners, their local rows, the pool of local rows): the boundaries live in local-row space -- the
    rows of a partition's [rows][32] fp32 lines and of the state's [rows][16] -- so the pool is big_table.pool over
    a partition's rows (the first and last 64, 64 round every boundary, closed under the truncation models), taken
    on every owner and mapped back to ids: id = p^-1(local N + owner), p the owner permutation (key 0: identity;
    shard_ref.owner_perm, held to rmx.owner_hash when the shard is made)."""
    rows = -(-SHARD_V // N)
    lp = bt.pool(rows, SHARD_K, SHARD_FORMS)
    loc = np.repeat(lp.ids, N)
    own = np.tile(np.arange(N, dtype=np.int64), len(lp.ids))
    keep = loc * N + own < SHARD_V
    loc, own = loc[keep], own[keep]
    ids = shard_ref.owner_perm(loc * N + own, key, SHARD_V, inverse=True)
    order = np.argsort(ids)
    return ids[order], own[order], loc[order], lp


def local_ids(rows_lo, rows_hi, N, key):
    """(ids, owners, local rows) of the local rows [rows_lo, rows_hi) of every owner."""
    loc = np.repeat(np.arange(rows_lo, rows_hi, dtype=np.int64), N)
    own = np.tile(np.arange(N, dtype=np.int64), rows_hi - rows_lo)
    keep = loc * N + own < SHARD_V
    return shard_ref.owner_perm((loc * N + own)[keep], key, SHARD_V, inverse=True), own[keep], loc[keep]


class Shard:
    def __init__(self, ctx, N, how):
        self.ctx, self.N = ctx, N
        self.key = 0 if how == "key0" else rmx.OWNER_HASH_DEFAULT
        self.t = bt.TABLES["T16"]
        self.rows = -(-SHARD_V // N)
        self.sh = self.twin = None
        try:
            self.sh = rmx.ShardedTable(ctx, SHARD_V, SHARD_K, N)
            if how == "key0":
                self.sh.set_owner_hash(0)
            self.sh.fill_synthetic(bt.SEED_TAB)
        except rmx.RmxError as e:
            self.close()
            if e.args and e.args[0] == _lib.RMX_E_NOMEM:
                pytest.skip("RMX_E_NOMEM: no room for the shard (%s)" % e)
            raise
        under_cap()
        assert self.sh.local_rows() == self.rows
        self.ids, self.own, self.loc, self.lp = shard_pool(N, self.key)
        self.bounds = self.lp.bounds
        for i in range(0, len(self.ids), 5):  # the restated permutation is the library's
            assert rmx.owner_hash(self.key, SHARD_V, N, int(self.ids[i])) == (int(self.own[i]), int(self.loc[i]))
        self.w, self.e = bt.rows_of(self.t, self.ids)
        self.twin = rmx.EmbeddingTable(ctx, len(self.ids), SHARD_K)
        self.twin.upload(self.w, self.e)

    def batch(self, B, F, seed):
        """every sample: one id at or above the partition's top boundary, one local row below 2^20"""
        rng = np.random.default_rng(seed)
        hi, lo = np.nonzero(self.loc >= self.bounds[-1])[0], np.nonzero(self.loc < bt.LOW)[0]
        r = rng.integers(0, len(self.ids), (B, F))
        r[:, 0] = hi[rng.integers(0, len(hi), B)]
        r[:, 1] = lo[rng.integers(0, len(lo), B)]
        return self.ids[r].astype(np.int32), r.astype(np.int32)

    def gather(self, ids):
        ctx, n = self.ctx, len(ids)
        ids_d = dev(ctx, np.asarray(ids).astype(np.int32))
        w_d, e_d = rmx.DeviceArray(ctx, n, np.float32), rmx.DeviceArray(ctx, n * SHARD_K, np.float32)
        self.sh.gather(ids_d, n, w_d, e_d)
        ctx.sync()
        out = w_d.numpy(), e_d.numpy().reshape(n, SHARD_K)
        for a in (ids_d, w_d, e_d):
            a.free()
        return out

    def check_untouched(self, touched, what, opt=None):
        """The places a truncated write would land, in local-row space: the alias windows (+- 1 row) of the touched
        ids' local rows in the partition's lines and in the state, and the pool's local rows with their neighbours,
        on every owner (the ids there gathered from the shard); and 64 random windows of 4,096 ids through
        download_rows.  Outside `touched` all hold the generator's bits; the optimiser's state there, read through
        shard_state_ptrs at the local rows and in 64 random windows of 4,096 local rows per owner, holds zeros."""
        N = self.N
        rng = np.random.default_rng(len(touched) + N)
        touched = np.unique(np.asarray(touched, np.int64))
        p_t = shard_ref.owner_perm(touched, self.key, SHARD_V) if len(touched) else touched
        spans = alias_spans(p_t // N, SHARD_K, SHARD_FORMS, self.rows)
        spans += [(max(a - 1, 0), min(a + n + 1, self.rows)) for a, n in bt.runs(self.lp.ids)]
        ids, own, loc = (np.concatenate(x) for x in zip(*[local_ids(a, b, N, self.key) for a, b in spans]))
        keep = ~np.isin(ids, touched)
        w, e = self.gather(ids)
        w_ref, e_ref = bt.rows_of(self.t, ids)
        assert same_bits(w[keep], w_ref[keep]) and same_bits(e[keep], e_ref[keep]), what + ": rows at alias windows"
        for r in rng.integers(0, SHARD_V - 4096, 64):
            win = np.arange(int(r), int(r) + 4096)
            k2 = ~np.isin(win, touched)
            w, e, owned = self.sh.download_rows(int(r), 4096)
            w_ref, e_ref = bt.rows_of(self.t, win)
            assert owned.all() and same_bits(w[k2], w_ref[k2]) and same_bits(e[k2], e_ref[k2]), (
                "%s: rows changed in ids [%d, %d)" % (what, r, r + 4096))
        if opt is None:
            return
        t_key = set((p_t % N * (1 << 40) + p_t // N).tolist())  # (owner, local row) of the touched ids
        for o in range(N):
            pw, pe = opt.shard_state_ptrs(0, o)
            wins = spans + [(int(r), int(r) + 4096) for r in rng.integers(0, self.rows - 4096, 64)]
            for a, b in wins:
                sw = rmx.DeviceArray(self.ctx, b - a, np.float32, ctypes.c_void_p(pw + 4 * a), opt).numpy()
                se = rmx.DeviceArray(self.ctx, (b - a) * SHARD_K, np.float32,
                                     ctypes.c_void_p(pe + 4 * SHARD_K * a), opt).numpy().reshape(b - a, SHARD_K)
                k3 = np.array([o * (1 << 40) + l not in t_key for l in range(a, b)])
                assert not sw[k3].any() and not se[k3].any(), "%s: state written in local rows [%d, %d) of %d" % (
                    what, a, b, o)

    def close(self):
        for o in (self.twin, self.sh):
            if o is not None:
                o.close()


SHARD_ROW = "deepfm_f13k16_209x37"


def shard_gather_and_rows(ctx, shard):
    """ShardedTable.gather of the pool is the generator; upload_rows / download_rows across id ranges whose local
    rows straddle the boundaries come back, with every row owned (a loopback shard holds every partition), and
    nothing moves where a truncated write would have landed."""
    sh = shard.sh
    w, e = shard.gather(shard.ids)
    assert same_bits(w, shard.w) and same_bits(e, shard.e)
    rng = np.random.default_rng(5)
    top = shard.ids[shard.loc >= shard.bounds[-1]]
    ranges = [(max(0, min(int(i) - 150, SHARD_V - 300)), 300) for i in (top[0], top[-1])] + [(SHARD_V - 300, 300), (0, 300)]
    if shard.key == 0:  # ids around local boundary b are N b - ... : a contiguous id range crosses it on every owner
        ranges += [(b * shard.N - 300, 600) for b in shard.bounds]
    touched = np.concatenate([np.arange(a, a + cnt) for a, cnt in ranges])
    try:
        for a, cnt in ranges:
            w = rng.uniform(-0.05, 0.05, cnt).astype(np.float32)
            e = rng.uniform(-0.05, 0.05, (cnt, SHARD_K)).astype(np.float32)
            assert sh.upload_rows(a, w, e) == cnt
            gw, ge, owned = sh.download_rows(a, cnt)
            assert owned.all() and same_bits(gw, w) and same_bits(ge, e), a
        shard.check_untouched(touched, "shard upload_rows")
    finally:
        for a, cnt in ranges:
            w, e = bt.rows_of(shard.t, np.arange(a, a + cnt))
            sh.upload_rows(a, w, e)
    w, e = shard.gather(shard.ids)  # the restore put the rows back
    assert same_bits(w, shard.w) and same_bits(e, shard.e)
    under_cap()


def shard_forward_and_backward(ctx, shard, dedupe):
    """forward_ids_sharded, pull + forward_pulled and backward_pulled: the bits of the replicated compact twin
    (include/rmx.h: a sharded table computes what a replicated one holding the same rows does, bit for bit)."""
    c, B = bt.case(SHARD_ROW), 300
    ids, ranks = shard.batch(B, c.F, 21)
    shard.sh.set_dedupe(dedupe)
    m_a, m_b = bt.rmx_model(SHARD_ROW, SHARD_V), bt.rmx_model(SHARD_ROW, len(shard.ids))
    a, b = dev(ctx, ids.reshape(-1)), dev(ctx, ranks.reshape(-1))
    out = rmx.DeviceArray(ctx, B, np.float32)
    bw = Backward(ctx, c, B, c.k, len(bt.host_mats(SHARD_ROW)))
    try:
        ref = run_reads(ctx, m_b, shard.twin, B, b)[1]["forward_ids"]
        m_a.forward_ids_sharded(shard.sh, B, a, out)
        ctx.sync()
        assert same_bits(out.numpy(), ref), "forward_ids_sharded"
        out.upload(np.full(B, np.nan, np.float32))
        shard.sh.pull(a, B * c.F, 1)
        m_a.forward_pulled(shard.sh, B, 1, out)
        ctx.sync()
        assert same_bits(out.numpy(), ref), "pull + forward_pulled"
        w, e = bt.rows_of(shard.t, ids.reshape(-1))
        err = float(np.abs(ref - bt.oracle_rows(SHARD_ROW, w, e.ravel(), 1)).max())
        assert err <= sc.TOL, err
        _, g_ref = bw.run(m_b, shard.twin, b)
        for o, nan in zip(bw.outs, bw.nans):
            o.upload(nan)
        shard.sh.pull(a, B * c.F, 0)
        g = bw.outs
        m_a.backward_pulled(shard.sh, B, 0, bw.targets, g[0], g[1], g[2], g[3], g[4])
        ctx.sync()
        for i, (o, r) in enumerate(zip(bw.outs, g_ref)):
            assert same_bits(o.numpy(), r), "backward_pulled output %d" % i
    finally:
        shard.sh.set_dedupe("auto")
        for o in (a, b, out, bw, m_a, m_b):
            o.close()
    under_cap()


def shard_train_steps(ctx, shard):
    """Three train_step_sharded with Adagrad (one state slot): losses, rows and the state of every pool id, read
    through shard_state_ptrs at the id's local row, equal the replicated twin's bit for bit; afterwards nothing has
    moved, in the rows or in the state, where a truncated push would have landed."""
    c, B, n = bt.case(SHARD_ROW), 64, len(shard.ids)
    m_a, m_b = bt.rmx_model(SHARD_ROW, SHARD_V), bt.rmx_model(SHARD_ROW, n)
    o_a = o_b = None
    touched = set()
    ids_d = dev(ctx, shard.ids.astype(np.int32))
    w_d, e_d = rmx.DeviceArray(ctx, n, np.float32), rmx.DeviceArray(ctx, n * SHARD_K, np.float32)
    try:
        o_a, o_b = rmx.Optimizer(m_a, shard.sh, "adagrad", eta=0.05), rmx.Optimizer(m_b, shard.twin, "adagrad", eta=0.05)
        under_cap()
        at = {(int(o), int(l)): i for i, (o, l) in enumerate(zip(shard.own, shard.loc))}
        for step in range(3):
            ids, ranks = shard.batch(B, c.F, 30 + step)
            touched |= set(ids.reshape(-1).tolist())
            a, b, tg = dev(ctx, ids.reshape(-1)), dev(ctx, ranks.reshape(-1)), dev(ctx, sc.host_targets(B))
            la = m_a.train_step_sharded(shard.sh, o_a, B, a, tg)
            lb = m_b.train_step_ids(shard.twin, o_b, B, b, tg)
            assert np.float32(la) == np.float32(lb) and np.isfinite(la), step
            shard.sh.gather(ids_d, n, w_d, e_d)
            ctx.sync()
            tw, te = shard.twin.download()
            assert same_bits(w_d.numpy(), tw) and same_bits(e_d.numpy(), te), "rows after step %d" % (step + 1)
            assert same_bits(m_a.getMats(), m_b.getMats())
            sw, se, _ = o_b.state_download_rows(0, 0, n)
            for o in range(shard.N):  # the state at the local row of every pool id, straight from the device
                pw, pe = o_a.shard_state_ptrs(0, o)
                for l0, cnt in bt.runs(shard.lp.ids):
                    idx = np.array([at.get((o, l), -1) for l in range(l0, l0 + cnt)])
                    gw = rmx.DeviceArray(ctx, cnt, np.float32, ctypes.c_void_p(pw + 4 * l0), o_a).numpy()
                    ge = rmx.DeviceArray(ctx, cnt * SHARD_K, np.float32,
                                         ctypes.c_void_p(pe + 4 * SHARD_K * l0), o_a).numpy().reshape(cnt, SHARD_K)
                    ok = idx >= 0
                    assert same_bits(gw[ok], sw[idx[ok]]) and same_bits(ge[ok], se[idx[ok]]), (step, o, l0)
            for o in (a, b, tg):
                o.free()
        tw, _ = shard.twin.download()
        assert not same_bits(tw, shard.w)  # the steps did move the rows
        shard.check_untouched(sorted(touched), "train_step_sharded", o_a)
    finally:
        for o in (o_a, o_b):
            if o is not None:
                o.close()
        for o in (m_a, m_b, ids_d, w_d, e_d):
            o.close()
        for a, cnt in bt.runs(np.array(sorted(touched), np.int64)):
            w, e = bt.rows_of(shard.t, np.arange(a, a + cnt))
            shard.sh.upload_rows(a, w, e)
        shard.twin.upload(shard.w, shard.e)
    under_cap()


# ---- one class per big table: the table lives while the class runs, one at a time ----------------------------
def table_class(cfg):
    reads, bwds = cases_of(cfg, bt.READ_CASES), cases_of(cfg, bt.BWD_CASES, BWD_KEY)

    class C:
        @pytest.fixture(scope="class")
        def big(self, ctx):
            yield from held(ctx, lambda: Big(ctx, *cfg), cfg_id(cfg))

        def test_gather_of_the_pool_is_the_generator(self, ctx, big):
            gather_of_the_pool_is_the_generator(ctx, big)

        @pytest.mark.parametrize("case", reads)
        def test_read_paths(self, ctx, ncu, big, case):
            read_paths(ctx, ncu, big, case)

        if bwds:
            @pytest.mark.parametrize("case", bwds)
            def test_backward_paths(self, ctx, ncu, big, case):
                backward_paths(ctx, ncu, big, case)

        if not cfg[1]:
            def test_nan_leftovers(self, ctx, big):
                nan_leftovers(ctx, big)

        @pytest.mark.parametrize("chunk", [300, None], ids=["chunk300", "chunk-default"])
        @pytest.mark.parametrize("layout", [rmx.LAYOUT_ROW_MAJOR, rmx.LAYOUT_K_MAJOR], ids=["row-major", "k-major"])
        def test_param_io_across_the_boundaries(self, ctx, big, layout, chunk):
            param_io_across_the_boundaries(ctx, big, layout, chunk)

        if cfg in OPT_KINDS:
            @pytest.mark.parametrize("kind", OPT_KINDS[cfg])
            def test_optimiser_steps(self, ctx, big, kind):
                optimiser_steps(ctx, big, kind)

    C.__name__ = C.__qualname__ = "Test_" + cfg_id(cfg).replace("-", "_")
    C.__doc__ = "%s: %s" % (cfg_id(cfg), Big.__doc__)
    return C


def shard_class(N, how):
    class C:
        @pytest.fixture(scope="class")
        def shard(self, ctx):
            yield from held(ctx, lambda: Shard(ctx, N, how), "the shard N = %d, %s" % (N, how))

        def test_shard_gather_and_rows(self, ctx, shard):
            shard_gather_and_rows(ctx, shard)

        @pytest.mark.parametrize("dedupe", [False, True], ids=["plain", "dedupe"])
        def test_shard_forward_and_backward(self, ctx, shard, dedupe):
            shard_forward_and_backward(ctx, shard, dedupe)

        def test_shard_train_steps(self, ctx, shard):
            shard_train_steps(ctx, shard)

    C.__name__ = C.__qualname__ = "Test_shard_N%d_%s" % (N, how)
    return C


for _cfg in ALL_CFG:
    _c = table_class(_cfg)
    globals()[_c.__name__] = _c
for _s in SHARDS:
    _c = shard_class(*_s)
    globals()[_c.__name__] = _c
del _c


def test_worst_oracle_errors():
    """The worst anchor errors of the run, for DESIGN.md §4 (beside the sweep's 1.2e-7 and 2.2e-5)."""
    print("big tables: worst max |p - p64| %.3g (fp32), worst max |p - p_bf16 emulation| %.3g (bf16)"
          % (WORST["fp32"], WORST["bf16"]))
    assert WORST["fp32"] <= sc.TOL and WORST["bf16"] <= sc.TOL_BF16
