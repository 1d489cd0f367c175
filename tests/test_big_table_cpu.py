"""What must hold on the host for test_big_table.py (tables past 2^31 elements and 4 GiB offsets) to mean
something; no GPU is used here.

 - the vectorised oracle_ctypes.gen_rows is orc_gen_table, bit for bit (against the per-id loop);
 - the rows at which an offset crosses a 32-bit mark, per table and form, are the hand-written ones; the id pool
   straddles each, holds the first and last 64 rows and the rows a truncated offset lands on; every sample of a
   batch holds an id at or above the top boundary and one below 2^20;
 - a truncated read cannot return the right bits: for every pool id and truncation model, what lies at the truncated
   address of each fp32 element differs from that element.  bf16 rows hold about 1,500 distinct values (8 bits of
   mantissa in +-0.05), so single elements do collide: there every 16-byte window of a row differs, and the row
   in at least three quarters of its elements;
 - the wrong row shows at the project's bars: on the f64 oracle, one row per kind at B = 37 with the high ids'
   rows replaced by their byte-truncated aliases moves p by >= 10 TOL on every sample (HI_SHARE of the fields are
   high ids: the share is raised, never the factor lowered);
 - every path DESIGN.md §4 lists for the big tables has a parametrised case."""
import os
import re

import numpy as np
import pytest

import big_table as bt
import oracle_ctypes as oc
import shape_cases as sc

T = bt.TABLES


def test_gen_rows_is_the_per_id_loop():
    rng = np.random.default_rng(3)
    for k in (0, 1, 8, 10, 16, 32):
        V = 2 ** 31 - 1
        ids = np.concatenate([[0, 1, V - 1, 2 ** 27, 2 ** 30 + 5], rng.integers(0, V, 200)])
        w, e = oc.gen_rows(sc.SEED_TAB, V, k, ids)
        wl, el = oc.gen_rows_loop(sc.SEED_TAB, V, k, ids)
        assert w.dtype == wl.dtype == np.float32 and e.shape == el.shape == (len(ids) * k,)
        assert np.array_equal(w.view(np.uint32), wl.view(np.uint32)), k
        assert np.array_equal(e.view(np.uint32), el.view(np.uint32)), k
    wt, et = oc.gen_table(sc.SEED_TAB, 1000, 16, 2 ** 27 - 500, 1000)  # and a run of rows in one call
    w, e = oc.gen_rows(sc.SEED_TAB, 0, 16, np.arange(2 ** 27 - 500, 2 ** 27 + 500))
    assert np.array_equal(w, wt) and np.array_equal(e.reshape(-1, 16), et)


BOUNDS = {
    ("T16", "f32"): (2 ** 26, 2 ** 27),              # 2^32 B; 2^31 elements = 2^33 B
    ("T16", "lines_f32"): (2 ** 25, 2 ** 26, 2 ** 27),   # 2^32 B; 2^31 el = 2^33 B; 2^32 el = 2^34 B
    ("T16", "bf16"): (2 ** 27,),                     # 2^31 elements = 2^32 B
    ("T16", "lines_bf16"): (2 ** 26, 2 ** 27),       # 2^31 el = 2^32 B; 2^32 el = 2^33 B
    ("T32", "f32"): (2 ** 25, 2 ** 26, 2 ** 27),
    ("T32", "bf16"): (2 ** 26, 2 ** 27),
    ("T8", "f32"): (2 ** 27, 2 ** 28),               # 2^32 B; 2^31 elements = 2^33 B
    ("T8", "bf16"): (2 ** 28,),
    ("T10", "f32"): (107374183, 214748365),          # ceil(2^32 / 40); ceil(2^31 / 10) = ceil(2^33 / 40)
    ("T10", "bf16"): (214748365,),
    ("T1", "f32"): (2 ** 30,),                       # 2^32 B only
    ("T1", "bf16"): (),
}


def test_tables_and_boundaries():
    assert [(t.k, t.V) for t in (T["T16"], T["T32"], T["T8"], T["T10"], T["T1"])] == [
        (16, 135266304), (32, 135266304), (8, 269484032), (10, 215796941), (1, 1074790400)]
    assert all(t.V < 2 ** 31 for t in T.values())
    for (name, form), want in BOUNDS.items():
        assert bt.boundaries(T[name].V, T[name].k, form) == want, (name, form)
    # sizes: fp32 dense 8.7 GB, the line copy 17.3 GB, bf16 dense 4.3 GB; T10's mark falls inside a row
    assert 16 * 4 * T["T16"].V > 2 ** 33 and 32 * 4 * T["T16"].V > 2 ** 34 and 16 * 2 * T["T16"].V > 2 ** 32
    assert 2 ** 31 % 10 and (214748365 - 1) * 10 < 2 ** 31 < 214748365 * 10


CONFIGS = [(n, b, l) for n, b, l in bt.configs()]


@pytest.mark.parametrize("name,bf16,lines", CONFIGS)
def test_pool_and_batches(name, bf16, lines):
    t = T[name]
    forms = bt.forms_of(t, bf16, lines)
    p = bt.pool_of(t, bf16, lines)
    assert np.all(np.diff(p.ids) > 0) and p.ids[0] == 0 and p.ids[-1] == t.V - 1
    have = set(p.ids.tolist())
    assert set(range(64)) <= have and set(range(t.V - 64, t.V)) <= have
    for f in forms:
        for b in bt.boundaries(t.V, t.k, f):
            assert set(range(b - 32, b + 32)) <= have, (f, b)
        assert set(bt.alias_rows(p.ids, t.k, f).tolist()) <= have, f  # closed under the truncation models
    assert p.top == max(p.bounds) and len(p.hi) >= 64 and len(p.lo) >= 64
    assert len(p.ids) < 2000
    for F, B in ((1, 37), (2, 37), (7, 300), (39, 16400)):
        ids = bt.batch_ids(p, B, F, 5)
        assert ids.shape == (B, F) and ids.dtype == np.int32 and bt.keeps_rule(p, ids), (F, B)
        r = bt.rank(p, ids)
        assert r.max() < len(p.ids) and np.array_equal(p.ids[r], ids)
    assert not bt.keeps_rule(p, np.zeros((4, 3), np.int64))


@pytest.mark.parametrize("name,bf16,lines", CONFIGS)
def test_truncated_reads_return_other_bits(name, bf16, lines):
    t = T[name]
    p = bt.pool_of(t, bf16, lines)
    moved = 0
    for form in bt.forms_of(t, bf16, lines):
        s, e = bt.stride(t.k, form), bt.esize(form)
        idx = p.ids[:, None] * s + np.arange(bt.used(t.k, form))[None, :]
        true = bt.flat_values(t, form, idx)
        for model in bt.MODELS:
            a = bt.truncate(idx, e, model)
            m = (a >= 0) & (a != idx)
            if not m.any():
                continue
            moved += int(m.sum())
            diff = bt.flat_values(t, form, np.where(m, a, idx)) != true
            if e == 4:
                assert diff[m].all(), (form, model, int((~diff[m]).sum()))
            else:  # 16-byte windows of 8 bf16 elements (the weight at 16 of a line is a window of its own)
                rows = m.all(1)
                for c0 in range(0, idx.shape[1], 8):
                    assert diff[rows, c0:c0 + 8].any(1).all(), (form, model, c0)
                assert (4 * diff[rows].sum(1) >= 3 * diff.shape[1]).all(), (form, model)
                assert (m.all(1) == m.any(1)).all() or t.k % 8, (form, model)  # (T10: a row the mark cuts)
    assert moved > 0


# ---- the wrong row at the project's bars ----------------------------------------------------------------------
HI_SHARE = 0.5
VISIBLE = (("deepfm_f7k10_33x20", "T10", "f32"), ("dnn_f17k8_500x7", "T8", "f32"), ("dcn_f17k16_64x32_d3", "T16", "f32"),
           ("pnn_f16k16_48x32", "T16", "f32"), ("xdeepfm_f41k16_33_cin5", "T16", "f32"),
           ("lr_f65k16", "T16", "lines_f32"), ("deepfm_f13k16_209x37", "T16", "lines_f32"))


@pytest.mark.parametrize("row,name,form", VISIBLE)
def test_truncated_rows_move_p_by_ten_bars(row, name, form):
    """Measured at HI_SHARE 0.5 (min / median over the 37 samples): deepfm_f7k10 3.1e-4 / 3.3e-3, dnn_f17k8 1.7e-4 /
    3.4e-3, dcn_f17k16 4.0e-4 / 8.7e-3, pnn_f16k16 1.9e-4 / 3.4e-3, xdeepfm_f41k16 1.5e-4 / 6.7e-3, lr_f65k16 2.9e-3 /
    4.3e-2, deepfm_f13k16 on lines 1.5e-3 / 2.2e-2.  The minimum is the sample whose change happens to pass nearest
    zero, and the share of high ids does not move it (xdeepfm_f5k16_100x37_cin10x7: 1.7e-5 at 0.5, 0.75 and 1.0,
    median 3e-3), so the xDeepFM row here is the F = 41 one."""
    t, c, B = T[name], sc.BY_NAME[row], 37
    p = bt.pool(t.V, t.k, (form,))
    ids = bt.batch_ids(p, B, c.F, 11, HI_SHARE).reshape(-1)
    w, e = bt.rows_of(t, ids)
    base = bt.oracle_rows(row, w, e.ravel(), 1).astype(np.float64)
    high = ids >= p.top
    wa, ea = bt.truncated_row(t, form, ids[high], "byte32")
    w2, e2 = w.copy(), e.copy()
    w2[high], e2[high] = wa, ea
    assert not np.array_equal(e2[high], e[high]) or c.kind == "lr"
    moved = np.abs(bt.oracle_rows(row, w2, e2.ravel(), 1).astype(np.float64) - base)
    print("%s on %s %s, %.0f %% high ids: min over the samples of |dp| = %.3g (bar %.0e)"
          % (row, name, form, 100 * high.mean(), moved.min(), sc.TOL))
    assert moved.min() >= 10 * sc.TOL, (row, float(moved.min()))


# ---- the table of DESIGN.md ------------------------------------------------------------------------------------
def test_every_listed_path_has_a_case():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    sect = text[text.index("<!-- big-table paths -->"):text.index("<!-- /big-table paths -->")]
    rows = [ln.strip() for ln in sect.splitlines() if ln.strip().startswith("|")]
    listed = [re.split(r"\s*\|\s*", ln.strip("|").strip())[0] for ln in rows[2:]]  # (after the header and its rule)
    listed = {p.strip("` ") for p in listed}
    assert listed == set(bt.all_paths()), (sorted(listed - set(bt.all_paths())), sorted(set(bt.all_paths()) - listed))
    import test_big_table as tb
    assert set(bt.OTHER_PATHS) == set(tb.PATH_TESTS)
    for path, (cls, test) in tb.PATH_TESTS.items():  # the paths without a case list: the test that runs each exists
        assert callable(getattr(getattr(tb, cls, None), test, None)), "%s: no %s::%s" % (path, cls, test)
    classes = {n: c for n, c in vars(tb).items() if n.startswith("Test_")}
    for r in bt.READ_CASES:  # ... and every case is a parameter of its table's class
        cls = classes["Test_" + tb.cfg_id((r.table, r.bf16, r.lines)).replace("-", "_")]
        marks = [m for m in cls.test_read_paths.pytestmark if m.name == "parametrize"]
        assert any(p.values[0] is r for p in marks[0].args[1]), r
    for b in bt.BWD_CASES:
        cls = classes["Test_" + tb.cfg_id((b.table, False, 0)).replace("-", "_")]
        marks = [m for m in cls.test_backward_paths.pytestmark if m.name == "parametrize"]
        assert any(p.values[0] is b for p in marks[0].args[1]), b
    for r in bt.READ_CASES:
        t = T[r.table]
        assert bt.case(r.row).k in (t.k, 16 if bt.case(r.row).kind == "lr" else t.k), r
        assert (r.table, r.bf16, r.lines) in bt.configs()
        assert bt.boundaries(t.V, t.k, "bf16" if r.bf16 else "f32"), r
    for b in bt.BWD_CASES:
        assert bt.case(b.row).k in (T[b.table].k, 16) and not sc.backward_refused(bt.case(b.row))


def test_cases_reach_their_paths():
    """Every claim of a case -- the REACH tag, the batch-selected tile (FWD_PRED / BF16_PRED / BWD_PRED), how layer 1
    forms A -- holds at 256 CUs; test_big_table.py evaluates them again on the device's CU count.  The gathers that
    differ by tile are each claimed: the split GEMM's narrow2, 8-wave and MT = 2 (id ring) tiles at k = 16, its 8-wave
    tile at k = 8, the f32 and bf16 engines' small and large tiles, the CIN's 2-wave and MT = 2 tiles."""
    claimed = set()
    for r in bt.READ_CASES:
        assert r.claims or bt.case(r.row).kind == "lr" or r.cin16 or r.path.startswith(("tail_fo", "lines lr")), r
        for cl in r.claims:
            assert bt.holds(cl, bt.case(r.row), r.B, sc.NCU, r.bf16), (r.path, r.row, r.B, cl)
            claimed.add(cl)
    for b in bt.BWD_CASES:
        for cl in b.claims:
            assert bt.holds(cl, bt.case(b.row), b.B, sc.NCU), (b.path, b.row, b.B, cl)
            claimed.add(cl)
    need = {"s3_narrow2", "s3_wave8", "s3_mt2_gather", "s3_wave8_gather_any", "f32_small4", "bf16_small4",
            "bf16_large_gather", "cin_2w", "cin_mt2", "cin_f32_lt_8192", "emb_fused", "layer1_k16", "layer1_any",
            "layer1_dense", "cols32", "gather_x_fp32", "gather_x_bf16", "gather_any_fp32", "gather_any_bf16",
            "encoder_generic", "cross_generic", "cross16_40", "dcn_fused", "product_generic", "product16_ntile2", "k_1"}
    assert need <= claimed, sorted(need - claimed)
