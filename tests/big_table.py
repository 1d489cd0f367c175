"""Tables past 2^31 elements and 4 GiB offsets (test_big_table_cpu.py, test_big_table.py): the tables, the rows at
which an offset into them crosses a 32-bit mark, the pool of ids around those rows and around the rows a
truncated offset would land on, batches drawn from the pool, and the compact twin -- a table of len(pool) rows
whose row r holds pool[r]'s row, generated on the host (oracle_ctypes.gen_rows), in which no 32-bit arithmetic
can alias.  The host never holds a whole table.

A form is one layout a table's rows are read in: `s` elements of `e` bytes between two rows.
    f32         dense fp32 rows                         s = k,  e = 4
    bf16        dense bf16 rows                         s = k,  e = 2
    lines_f32   the [emb 16 | w | pad 15] line copy      s = 32, e = 4   (k = 16, knob table_lines 1; a shard's
    lines_bf16  the same of a bf16 table                 s = 32, e = 2    partition at k = 16 is lines_f32)
The first-order weights [V] are s = 1: of the tables here only T1's cross a mark, at the row its k = 1 rows do.

READ_CASES / BWD_CASES name, per table kernel path, the (table, dtype, lines, row, batch) that test_big_table.py
runs; DESIGN.md §4 lists the same paths (test_big_table_cpu.py::test_every_listed_path_has_a_case)."""
import collections
import functools

import numpy as np

import oracle_ctypes as oc
import shape_cases as sc

SEED_TAB = sc.SEED_TAB
Table = collections.namedtuple("Table", "name k V")
TABLES = {t.name: t for t in (
    Table("T16", 16, 2 ** 27 + 2 ** 20), Table("T32", 32, 2 ** 27 + 2 ** 20), Table("T8", 8, 2 ** 28 + 2 ** 20),
    Table("T10", 10, -(-2 ** 31 // 10) + 2 ** 20), Table("T1", 1, 2 ** 30 + 2 ** 20))}
FORMS = ("f32", "bf16", "lines_f32", "lines_bf16")
ELEM_MARKS = (2 ** 31, 2 ** 32)
BYTE_MARKS = (2 ** 32, 2 ** 33, 2 ** 34)
MODELS = ("byte32", "elem32", "int32")  # offset in bytes mod 2^32, in elements mod 2^32, in elements as int32 >= 0
LOW = 2 ** 20
MEM_CAP = 40 << 30


def stride(k, form):
    return 32 if form.startswith("lines") else k


def esize(form):
    return 2 if form.endswith("bf16") else 4


def used(k, form):
    """elements of a row that hold something: the k embeddings, and the weight at 16 in a line"""
    return 17 if form.startswith("lines") else k


def forms_of(t, bf16=False, lines=True):
    f = ["bf16" if bf16 else "f32"]
    if t.k == 16 and lines:
        f.append("lines_bf16" if bf16 else "lines_f32")
    return tuple(f)


def boundaries(V, k, form):
    """Rows b < V at which b * s reaches 2^31 or 2^32 elements, or b * s * e reaches 2^32, 2^33 or 2^34 bytes."""
    s, e = stride(k, form), esize(form)
    rows = {-(-m // s) for m in ELEM_MARKS} | {-(-m // (s * e)) for m in BYTE_MARKS}
    return tuple(sorted(b for b in rows if 0 < b < V))


def truncate(idx, e, model):
    """The element index a 32-bit offset makes of element index idx (int64 array); -1 where the model does not
    apply (int32: the low 32 bits read as a negative number)."""
    idx = np.asarray(idx, np.int64)
    if model == "byte32":
        return (idx * e % 2 ** 32) // e
    low = idx % 2 ** 32
    return low if model == "elem32" else np.where(low < 2 ** 31, low, -1)


def alias_rows(ids, k, form):
    """The rows that hold the truncated address of the first and the last element of every id, for every
    truncation model that moves it."""
    s, e, ids = stride(k, form), esize(form), np.asarray(ids, np.int64)
    out = []
    for last in (0, used(k, form) - 1):
        idx = ids * s + last
        for m in MODELS:
            a = truncate(idx, e, m)
            out.append(a[(a >= 0) & (a != idx)] // s)
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


Pool = collections.namedtuple("Pool", "ids hi lo top bounds")


@functools.lru_cache(None)
def pool(V, k, forms):
    """Pool(ids ascending, the ids at or above the highest boundary, the ids below 2^20, that boundary, every
    boundary of the forms)."""
    bounds = tuple(sorted({b for f in forms for b in boundaries(V, k, f)}))
    assert bounds, (V, k, forms)
    base = [np.arange(0, 64), np.arange(V - 64, V)] + [np.arange(b - 32, b + 32) for b in bounds]
    base = np.unique(np.concatenate(base).astype(np.int64))
    ids = np.unique(np.concatenate([base] + [alias_rows(base, k, f) for f in forms]))
    assert ids[0] == 0 and ids[-1] == V - 1
    top = bounds[-1]
    return Pool(sc._ro(ids), sc._ro(ids[ids >= top]), sc._ro(ids[ids < LOW]), top, bounds)


def pool_of(t, bf16=False, lines=True):
    return pool(t.V, t.k, forms_of(t, bf16, lines))


def runs(ids):
    """[(first id, count)] of the runs of consecutive ids of an ascending array."""
    ids = np.asarray(ids, np.int64)
    cut = np.nonzero(np.diff(ids) != 1)[0] + 1
    return [(int(r[0]), len(r)) for r in np.split(ids, cut) if len(r)]


def batch_ids(p, B, F, seed, hi_share=0.5):
    """[B][F] int32 ids from the pool in any field order: a field is a high id with probability hi_share, else
    any pool id; then one field of every sample is made a high id and another a low one (F = 1: the samples
    alternate high, low)."""
    rng = np.random.default_rng(seed)
    ids = p.ids[rng.integers(0, len(p.ids), (B, F))]
    hi = p.hi[rng.integers(0, len(p.hi), (B, F))]
    ids = np.where(rng.random((B, F)) < hi_share, hi, ids)
    rows = np.arange(B)
    if F == 1:
        ids[0::2, 0] = p.hi[rng.integers(0, len(p.hi), len(rows[0::2]))]
        ids[1::2, 0] = p.lo[rng.integers(0, len(p.lo), len(rows[1::2]))]
    else:
        f_hi = rng.integers(0, F, B)
        f_lo = (f_hi + 1 + rng.integers(0, F - 1, B)) % F
        ids[rows, f_hi] = p.hi[rng.integers(0, len(p.hi), B)]
        ids[rows, f_lo] = p.lo[rng.integers(0, len(p.lo), B)]
    return np.ascontiguousarray(ids, np.int32)


def keeps_rule(p, ids):
    ids = np.asarray(ids, np.int64)
    if ids.shape[1] == 1:
        return bool((ids[0::2, 0] >= p.top).all() and (ids[1::2, 0] < LOW).all())
    return bool(((ids >= p.top).any(1) & (ids < LOW).any(1)).all() and np.isin(ids, p.ids).all())


def rank(p, ids):
    """The twin's ids: the rank of every id in the pool."""
    r = np.searchsorted(p.ids, np.asarray(ids, np.int64))
    assert np.array_equal(p.ids[r], np.asarray(ids, np.int64))
    return np.ascontiguousarray(r, np.int32)


def rows_of(t, ids, bf16=False):
    """(w [n], e [n][k]) of the ids, fp32 (bf16: rounded to nearest even, as fill_synthetic stores them)."""
    w, e = oc.gen_rows(SEED_TAB, t.V, t.k, np.asarray(ids, np.int64).reshape(-1))
    if bf16:
        w, e = oc.round_bf16(w), oc.round_bf16(e)
    return w, e.reshape(-1, t.k)


def flat_values(t, form, idx):
    """The values at element indices idx of the form's buffer, as fp32 (bf16 forms: rounded)."""
    s = stride(t.k, form)
    r, c = np.divmod(np.asarray(idx, np.int64), s)
    with np.errstate(over="ignore"):
        col = np.where(c < t.k, c, t.k)  # the weight is the generator's column k
        h = oc._splitmix64_np(np.uint64(SEED_TAB) ^ (r.astype(np.uint64) * np.uint64(t.k + 1) + col.astype(np.uint64)))
    v = oc._unif_np(h, 0.05)
    if form.startswith("lines"):
        v = np.where(c <= 16, v, np.float32(0))
    return oc.round_bf16(v).reshape(v.shape) if form.endswith("bf16") else v


def truncated_row(t, form, ids, model):
    """(w [n], e [n][k]) a reader of the form gets for the ids when its offsets go through the truncation model
    (elements the model leaves alone are the true ones).  The dense forms read w from [V]: s = 1."""
    ids = np.asarray(ids, np.int64)
    s, e = stride(t.k, form), esize(form)
    idx = ids[:, None] * s + np.arange(t.k)[None, :]
    a = truncate(idx, e, model)
    emb = flat_values(t, form, np.where(a >= 0, a, idx))
    if form.startswith("lines"):
        wi = ids * s + 16
        a = truncate(wi, e, model)
        w = flat_values(t, form, np.where(a >= 0, a, wi))
    else:
        a = truncate(ids, e, model)
        w = rows_of(t, np.where(a >= 0, a, ids), form.endswith("bf16"))[0]
    return w, emb


# ---- models: rows of shape_cases, and the benchmark towers at k = 16 -----------------------------------------
EXTRA = {c.name: c for c in (sc._c("deepfm", 39, 16, (400, 400, 400), ""), sc._c("dnn", 39, 16, (400, 400, 400), ""),
                             sc._c("pnn", 39, 16, (400, 400, 400), ""))}


def case(name):
    return sc.BY_NAME[name] if name in sc.BY_NAME else EXTRA[name]


@functools.lru_cache(None)
def orc_model(name):
    c = case(name)
    return oc.make_model(sc.ORC[c.kind], c.F, c.k, fc=c.fc, cin=c.cin, cross_depth=c.cross)


@functools.lru_cache(None)
def host_mats(name, bf16=False):
    if name in sc.BY_NAME:
        return sc.host_mats(name, bf16)
    mats = oc.init_mats(orc_model(name), sc.SEED_MATS)
    return sc._ro(oc.round_bf16(mats) if bf16 else mats)


def rmx_model(name, V, bf16=False, cin_bf16=False):
    import rmx
    c = case(name)
    fc, cin = list(c.fc), list(c.cin)
    m = {"lr": lambda: rmx.LR(V, c.F), "deepfm": lambda: rmx.DeepFM(V, c.F, c.k, fc),
         "dnn": lambda: rmx.DNN(V, c.F, c.k, fc), "dcn": lambda: rmx.DCN(V, c.F, c.k, c.cross, fc),
         "pnn": lambda: rmx.PNN(V, c.F, c.k, fc), "xdeepfm": lambda: rmx.XDeepFM(V, c.F, c.k, fc, cin)}[c.kind]()
    if bf16:
        m.setPrecision(rmx.DTYPE_BF16)
    if cin_bf16:
        m.setCinPrecision(rmx.DTYPE_BF16)
    if c.kind != "lr":
        m.setMats(host_mats(name, bf16))
    m.setBias(sc.BIAS)
    return m


def oracle_rows(name, w, e, precision, bf16=False):
    """The oracle's probabilities on gathered rows (w [B F], e [B F][k]): 1 f64, 2 the bf16 emulation."""
    c = case(name)
    B = len(w) // c.F
    lr = c.kind == "lr"
    return oc.forward(orc_model(name), B, sc.index_of(B, c.F), np.array([sc.BIAS], np.float32), w,
                      None if lr else e, None if lr else host_mats(name, bf16), precision)


# ---- the runs --------------------------------------------------------------------------------------------------
# (path, table, bf16, lines, row, batch, knobs, stages that must be in the stage list, cin bf16)
# claims: what must hold of (row, batch, CU count) for the run to reach the path it is named for -- names of
# shape_cases.REACH / FWD_PRED / BF16_PRED / BWD_PRED or of EXTRA_PRED below, held at 256 CUs on the CPU and
# re-evaluated on the device's CU count before the run; absent: stages that must not be in the stage list
Read = collections.namedtuple("Read", "path table bf16 lines row B knobs want cin16 claims absent")

EXTRA_PRED = {
    "layer1_k16": lambda c, B, n, bf16: sc.tower_layers(c, bf16)[0].amode == "k16",
    "layer1_any": lambda c, B, n, bf16: sc.tower_layers(c, bf16)[0].amode == "any",
    "layer1_dense": lambda c, B, n, bf16: sc.tower_layers(c, bf16)[0].amode == "dense",
    "cols32": lambda c, B, n, bf16: not bf16 and sc.cols32_path(c, B),
    "dcn_fused": lambda c, B, n, bf16: sc.dcn_fused(c),
    "row_owner_layer1": lambda c, B, n, bf16: sc.row_owner_candidate(c, 0, sc.tower_layers(c, bf16)[0]),
    "row_owner_tail": lambda c, B, n, bf16: all(sc.row_owner_candidate(c, i, L) for i, L in
                                                enumerate(sc.tower_layers(c, bf16)) if i > 0),
}


def holds(claim, c, B, ncu, bf16=False):
    """The claim at (case, batch, CU count)."""
    if claim in EXTRA_PRED:
        return bool(EXTRA_PRED[claim](c, B, ncu, bf16))
    if claim in sc.REACH:
        return bool(sc.REACH[claim](c))
    for preds in (sc.FWD_PRED, sc.BF16_PRED, sc.BWD_PRED):
        if claim in preds:
            return bool(preds[claim](c, B, ncu))
    raise KeyError(claim)


def _r(path, table, row, B, bf16=False, lines=0, knobs=(), want=(), cin16=False, claims="", absent=()):
    return Read(path, table, bf16, lines, row, B, tuple(knobs), tuple(want), cin16, tuple(claims.split()), tuple(absent))


D400, N400, P400 = "deepfm_f39k16_400x400x400", "dnn_f39k16_400x400x400", "pnn_f39k16_400x400x400"
READ_CASES = (
    # the encoder kernels: k = 16 at enc_u 0 / 13 / 20 (DeepFM column-split: the encoder stores x), the generic one
    _r("encoder_k16 enc_u 0", "T16", "deepfm_f13k16_209x37", 300, knobs=(("enc_u", 0),), want=("encoder_fm_x",), claims="cols32"),
    _r("encoder_k16v2 enc_u 13", "T16", "deepfm_f13k16_209x37", 300, knobs=(("enc_u", 13),), want=("encoder_fm_x",), claims="cols32"),
    _r("encoder_k16v2 enc_u 20", "T16", "deepfm_f13k16_209x37", 300, knobs=(("enc_u", 20),), want=("encoder_fm_x",), claims="cols32"),
    _r("encoder_k16v2 bf16", "T16", "deepfm_f13k16_209x37", 300, bf16=True, want=("encoder_fm",), claims="layer1_k16",
       absent=("encoder_fm_x",)),
    _r("encoder_generic", "T10", "deepfm_f7k10_33x20", 300, want=("encoder_fm", "gather_x"), claims="encoder_generic"),
    _r("encoder_generic", "T8", "deepfm_f17k8_500x7", 300, want=("encoder_fm",), claims="encoder_generic layer1_any",
       absent=("gather_x",)),
    _r("encoder_generic bf16", "T10", "deepfm_f7k10_33x20", 300, bf16=True, want=("encoder_fm", "gather_x"),
       claims="encoder_generic gather_x_bf16"),
    # x materialised (k % 4 != 0; bf16: k % 8 != 0) and the engines' gather at k != 16
    _r("gather_x fp32", "T10", "dnn_f7k10_33x20", 300, want=("gather_x",), claims="gather_x_fp32 layer1_dense"),
    _r("gather_x fp32", "T1", "deepfm_f2k1_5x3", 300, want=("gather_x",), claims="gather_x_fp32 k_1 layer1_dense"),
    _r("gather_x bf16", "T10", "dnn_f7k10_33x20", 300, bf16=True, want=("gather_x",), claims="gather_x_bf16 layer1_dense"),
    _r("gather_any fp32", "T8", "dnn_f17k8_500x7", 300, claims="gather_any_fp32 layer1_any f32_small4",
       absent=("gather_x",)),
    _r("gather_any fp32", "T32", "dnn_f3k32_520", 300, claims="gather_any_fp32 layer1_any f32_small4", absent=("gather_x",)),
    _r("gather_any fp32 large tiles", "T8", "dnn_f17k8_400x400x400", 16400, want=("tower_tail",),
       claims="gather_any_fp32 layer1_any s3_wave8_gather_any", absent=("gather_x",)),
    _r("gather_any bf16", "T8", "dnn_f17k8_500x7", 300, bf16=True, claims="gather_any_bf16 layer1_any bf16_small4",
       absent=("gather_x",)),
    # k = 16 rows gathered by the split-GEMM tiles and the bf16 engine
    _r("s3 gather narrow2", "T16", "deepfm_f13k16_401x37", 2049, want=("tower_layer1",),
       claims="layer1_k16 deepfm_fm_fused_layer1 s3_narrow2", absent=("encoder_fm", "encoder_fm_x")),
    _r("s3 gather 8-wave", "T16", "deepfm_f13k16_401x37", 16400, want=("tower_layer1",),
       claims="layer1_k16 deepfm_fm_fused_layer1 s3_wave8", absent=("encoder_fm", "encoder_fm_x")),
    # the MT = 2 tile (16 waves), the only one that addresses rows from the id ring
    _r("s3 gather 16-wave / MT 2", "T16", "deepfm_f39k16_832x200", 16400, want=("tower_layer1",),
       claims="layer1_k16 deepfm_fm_fused_layer1 s3_mt2_gather", absent=("encoder_fm", "encoder_fm_x")),
    _r("f32 engine gather k16", "T16", "dnn_f9k16_24x8x200x7x16", 300, claims="layer1_k16 f32_small4", absent=("gather_x",)),
    _r("bf16 engine gather k16", "T16", "dcn_f17k16_64x32_d3", 300, bf16=True, claims="layer1_k16 bf16_small4",
       absent=("gather_x",)),
    _r("bf16 engine gather k16 large tiles", "T16", "dcn_f17k16_64x32_d3", 65573, bf16=True,
       claims="layer1_k16 bf16_large_gather", absent=("gather_x",)),
    # the row-owner kernels
    _r("tower_fused", "T16", D400, 16400, want=("tower_fused",), claims="row_owner_layer1 row_owner_tail"),
    _r("head_s3 (s3_head 2)", "T16", D400, 16400, knobs=(("s3_small", 0), ("s3_fused", 0), ("s3_head", 2), ("s3_tail", 2)),
       want=("tower_layer1", "tower_tail"), claims="row_owner_layer1 row_owner_tail",
       absent=("encoder_fm", "encoder_fm_x", "first_order", "tower_fused", "tower_layer2")),
    _r("tail_s3", "T16", N400, 16400, want=("tower_layer1", "tower_tail"), claims="layer1_k16 row_owner_tail",
       absent=("tower_layer2",)),
    _r("tail_s3", "T16", "deepfm_f41k16_400x400x400", 16400, want=("encoder_fm", "tower_layer1", "tower_tail"),
       claims="F_41 layer1_k16 row_owner_tail", absent=("tower_layer2",)),
    _r("tower_small rt 1", "T16", D400, 4096, knobs=(("s3_small", 2), ("s3_small_rt", 1)), want=("tower_small",),
       claims="row_owner_layer1 row_owner_tail"),
    _r("tower_small rt 2", "T16", D400, 4096, knobs=(("s3_small", 2), ("s3_small_rt", 2)), want=("tower_small",),
       claims="row_owner_layer1 row_owner_tail"),
    _r("column-split", "T16", D400, 2048, want=("encoder_fm_x",), claims="cols32"),
    _r("column-split", "T16", "deepfm_f40k16_400x400x400", 300, want=("encoder_fm_x",), claims="cols32 F_40"),
    # the interactions
    _r("cross_kernel", "T10", "dcn_f7k10_33_d3", 300, want=("cross",), claims="cross_generic cross_generic_k_not_16"),
    _r("cross_kernel", "T8", "dcn_f17k8_32_d3", 300, want=("cross",), claims="cross_generic cross_generic_k_not_16"),
    _r("cross16_kernel", "T16", "dcn_f17k16_32_d3", 300, want=("cross",), claims="cross16_40"),
    _r("cross fused", "T16", "dcn_f17k16_64x32_d3", 300, claims="dcn_fused cross_fused_F_edge layer1_k16",
       absent=("cross", "gather_x")),
    _r("cross fused", "T10", "dcn_f7k10_33x20_d3", 300, want=("gather_x",), claims="dcn_fused gather_x_fp32",
       absent=("cross",)),
    _r("product_kernel", "T10", "pnn_f7k10_33x20", 300, want=("product",), claims="product_generic"),
    _r("product_kernel", "T8", "pnn_f17k8_500x7", 300, want=("product",), claims="product_generic"),
    _r("product16_kernel", "T16", "pnn_f17k16_48x32", 300, want=("product",), claims="product16_ntile2"),
    _r("product16_kernel bf16", "T16", "pnn_f17k16_48x32", 300, bf16=True, want=("product",), claims="product16_ntile2"),
    _r("cin x0 gather fp32", "T16", "xdeepfm_f5k16_100x37_cin10x7", 300, want=("cin_layer1",), claims="cin_f32_lt_8192"),
    _r("cin x0 gather split 2-wave", "T16", "xdeepfm_f5k16_33_cin200x7", 509, want=("cin_layer1",), claims="cin_split cin_2w"),
    _r("cin x0 gather split", "T16", "xdeepfm_f5k16_33_cin200x7", 4099, want=("cin_layer1",), claims="cin_split cin_mt2"),
    _r("cin x0 gather bf16", "T16", "xdeepfm_f5k16_33_cin200x7", 509, want=("cin_layer1",), cin16=True),
    _r("tail_fo (PNN bf16)", "T16", P400, 16400, bf16=True, want=("product", "tower_tail")),
    _r("lr", "T16", "lr_f65k16", 300, want=("first_order_sigmoid",)),
    _r("lr", "T1", "lr_f1k16", 300, want=("first_order_sigmoid",)),
    # the line copy: DeepFM, DNN, LR, fp32 and bf16
    _r("lines deepfm", "T16", "deepfm_f13k16_209x37", 300, lines=1, want=("encoder_fm_x",), claims="cols32"),
    _r("lines deepfm s3 gather", "T16", "deepfm_f13k16_401x37", 16400, lines=1, want=("tower_layer1",),
       claims="layer1_k16 deepfm_fm_fused_layer1 s3_wave8", absent=("encoder_fm", "encoder_fm_x")),
    _r("lines deepfm s3 gather MT 2", "T16", "deepfm_f39k16_832x200", 16400, lines=1, want=("tower_layer1",),
       claims="layer1_k16 deepfm_fm_fused_layer1 s3_mt2_gather", absent=("encoder_fm", "encoder_fm_x")),
    _r("lines deepfm tower_fused", "T16", D400, 16400, lines=1, want=("tower_fused",), claims="row_owner_layer1"),
    _r("lines dnn", "T16", "dnn_f9k16_24x8x200x7x16", 300, lines=1, claims="layer1_k16 f32_small4", absent=("gather_x",)),
    _r("lines lr", "T16", "lr_f65k16", 300, lines=1, want=("first_order_sigmoid",)),
    _r("lines deepfm bf16", "T16", "deepfm_f13k16_209x37", 300, bf16=True, lines=1, want=("encoder_fm",),
       claims="layer1_k16 bf16_small4"),
    _r("lines dnn bf16", "T16", "dnn_f9k16_24x8x200x7x16", 300, bf16=True, lines=1, claims="layer1_k16 bf16_small4",
       absent=("gather_x",)),
    _r("lines lr bf16", "T16", "lr_f65k16", 300, bf16=True, lines=1, want=("first_order_sigmoid",)),
)

# backward: the runs of shape_cases.BWD_RUNS that read the table differently (at the smallest batch that keeps the
# read: the dW tiles the batch picks never see the table), with the knobs that change the read
Bwd = collections.namedtuple("Bwd", "path table row B knobs claims want absent")


def _b(path, table, row, B, knobs=(), claims="", want=(), absent=()):
    return Bwd(path, table, row, B, tuple(knobs), tuple(claims.split()), tuple(want), tuple(absent))


BWD_CASES = (
    _b("backward emb_fused", "T16", "deepfm_f13k16_209x37", 2049, claims="emb_fused", want=("encoder_fm_x",),
       absent=("emb_grad",)),
    _b("backward emb_fused", "T16", "deepfm_f26k16_413x20", 2049, claims="emb_fused emb_fused_F_26",
       want=("encoder_fm_x",), absent=("emb_grad",)),
    _b("backward train_head_s3 1", "T16", D400, 4099, (("train_head_s3", 1),), "row_owner_layer1", ("head_x",),
       ("encoder_fm_x", "tower_layer1")),
    _b("backward train_head_s3 0", "T16", D400, 4099, (("train_head_s3", 0),), "row_owner_layer1",
       ("encoder_fm_x", "tower_layer1"), ("head_x",)),
    _b("backward enc_v2_x 1", "T16", "deepfm_f13k16_401x37", 300, (("enc_v2_x", 1),), "emb_fused", ("encoder_fm_x",)),
    _b("backward enc_v2_x 0", "T16", "deepfm_f13k16_401x37", 300, (("enc_v2_x", 0),), "emb_fused", ("encoder_fm_x",)),
    _b("backward dnn k16", "T16", "dnn_f9k16_24x8x200x7x16", 300, want=("gather_x", "emb_grad")),
    _b("backward pnn", "T16", "pnn_f17k16_48x32", 300, claims="product16_ntile2", want=("product", "emb_grad")),
    _b("backward dcn", "T16", "dcn_f17k16_64x32_d3", 300, want=("cross", "cross_back", "gather_x", "emb_grad")),
    _b("backward xdeepfm", "T16", "xdeepfm_f5k16_100x37_cin10x7", 300, want=("cin_back", "gather_x", "emb_grad")),
    _b("backward lr", "T16", "lr_f65k16", 300, want=("first_order_sigmoid",)),
    _b("backward generic k", "T10", "deepfm_f7k10_33x20", 300, claims="encoder_generic gather_x_fp32",
       want=("encoder_fm", "gather_x", "emb_grad")),
    _b("backward pnn generic k", "T10", "pnn_f7k10_33x20", 300, claims="product_generic", want=("product", "emb_grad")),
    _b("backward dcn generic k", "T10", "dcn_f7k10_33x20_d3", 300, claims="gather_x_fp32",
       want=("cross", "cross_back", "gather_x", "emb_grad")),
)

# the write paths and the rest, run by tests of their own (test_big_table.py names them in WRITE_PATHS)
OTHER_PATHS = ("rmx_gather", "rmx_gather bf16", "fill_synthetic / pack_lines", "param_io put / get rows",
               "param_io put rows into lines", "optim apply (tab_update)", "optim state put / get rows",
               "train_step_ids", "shard gather", "shard forward / pull", "shard put / get rows",
               "shard push (train_step_sharded)")


def configs():
    """(table, bf16, lines) of every big table the read and backward cases need, one alive at a time."""
    seen = []
    for r in READ_CASES:
        if (r.table, r.bf16, r.lines) not in seen:
            seen.append((r.table, r.bf16, r.lines))
    return sorted(seen)


def all_paths():
    return sorted({r.path for r in READ_CASES} | {b.path for b in BWD_CASES} | set(OTHER_PATHS))
