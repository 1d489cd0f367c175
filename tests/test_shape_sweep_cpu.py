"""What must be true of the reference alone for the off-benchmark sweep (shape_cases.py), so that a failure of
test_shape_sweep.py can only be the kernels': no GPU is used here.

For every row, at B = 128:
 - the fp32 oracle is within TOL / 2 of the f64 one (the GPU test holds the device to TOL of both);
 - bf16 rows: the bf16 emulation (stored activations rounded) is within TOL_BF16 / 2 of the f64 oracle on the same
   bf16-rounded parameters;
 - edge visibility: zeroing the last input column of a hidden Linear (PNN: of the product block too), or its last
   output unit with that unit's bias, moves some probability by at least 10 TOL (fp32) / 4 TOL_BF16 (bf16) -- a
   kernel that drops or mis-pads the edge of a layer fails its parity test by a wide margin instead of hiding in
   the noise.  A row whose output weights are too small for that is given a power-of-two `scale` on them; a row
   that cannot meet the bf16 factor has edge16 False in the table: the fp32 run is its edge check (it still runs
   in bf16, at the bf16 bar);
 - backward: 4 B candidate rows at B = 300 hold at least B rows free of ReLU ties;
and the table names a row for every path of shape_cases.REACH, by shape arithmetic that fails when a row is
edited away from it.

For the batch axis (test_batch_sweep.py): every batch-dependent predicate is claimed by a (row, batch) that a GPU
test runs; the 208 x 208 dW's slice count restated in Python is the library's; each backward run has B tie-free
rows among 4 B candidates; and leaving its last partial chunk out of the batch sums breaks the gradient bars."""
import numpy as np
import pytest

import shape_cases as sc

B_CPU = 128
VIS_FP32, VIS_BF16 = 10 * sc.TOL, 4 * sc.TOL_BF16
BF16_RUN = [n for n in sc.BF16_NAMES if not sc.bf16_refused(sc.BY_NAME[n])]


def visibility(name, bf16):
    """[(what, max |dp|)]: the oracle's response (f64, or the bf16 emulation on rounded parameters) to zeroing
    the edge column / unit of every hidden Linear of the row."""
    c = sc.BY_NAME[name]
    prec = 2 if bf16 else 1
    ids = sc.host_ids(c.F, B_CPU)
    base = sc.oracle_forward(name, B_CPU, prec, bf16).astype(np.float64)
    res = []
    lins, _ = sc.linears(c)
    for L in lins:
        m = sc.host_mats(name, bf16).copy()
        W = m[L.w_off:L.w_off + L.N * L.K].reshape(L.N, L.K)
        W[:, L.K - 1] = 0
        res.append((L.what + " last input column", float(np.abs(sc.oracle_on(c, ids, prec, bf16, m) - base).max())))
    for L in lins:
        if L.what == "layer1_product":
            continue  # the unit's two blocks go together, below
        m = sc.host_mats(name, bf16).copy()
        for L2 in lins:
            if L2 is L or (L.what == "layer1_x" and L2.what == "layer1_product"):
                m[L2.w_off:L2.w_off + L2.N * L2.K].reshape(L2.N, L2.K)[L2.N - 1, :] = 0
        if L.b_off is not None:
            m[L.b_off + L.N - 1] = 0
        res.append((L.what.replace("_x", "") + " last output unit",
                    float(np.abs(sc.oracle_on(c, ids, prec, bf16, m) - base).max())))
    return res


@pytest.mark.parametrize("name", sc.NAMES)
def test_fp32_reference_bar(name):
    p32 = sc.oracle_forward(name, B_CPU, 0)
    p64 = sc.oracle_forward(name, B_CPU, 1)
    err = float(np.abs(p32.astype(np.float64) - p64).max())
    print("%s: max |p32 - p64| = %.3g" % (name, err))
    assert np.isfinite(p64).all() and err <= sc.TOL / 2


@pytest.mark.parametrize("name", BF16_RUN)
def test_bf16_storage_rounding(name):
    p2 = sc.oracle_forward(name, B_CPU, 2, True)
    p1 = sc.oracle_forward(name, B_CPU, 1, True)
    err = float(np.abs(p2.astype(np.float64) - p1).max())
    print("%s: max |p(bf16 emulation) - p(f64)| on bf16 parameters = %.3g" % (name, err))
    assert err <= sc.TOL_BF16 / 2


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc.BY_NAME[n].kind != "lr"])
def test_edge_visibility_fp32(name):
    vis = visibility(name, False)
    print("%s: %s" % (name, ", ".join("%s %.3g" % v for v in vis)))
    assert vis and min(v for _, v in vis) >= VIS_FP32, vis


@pytest.mark.parametrize("name", [n for n in BF16_RUN if sc.BY_NAME[n].kind != "lr" and sc.BY_NAME[n].edge16])
def test_edge_visibility_bf16(name):
    vis = visibility(name, True)
    print("%s: %s" % (name, ", ".join("%s %.3g" % v for v in vis)))
    assert vis and min(v for _, v in vis) >= VIS_BF16, vis


@pytest.mark.parametrize("name", [n for n in sc.NAMES if not sc.backward_refused(sc.BY_NAME[n])])
def test_backward_tie_rule(name):
    B = 300
    keep = sc.tie_free_rows(name, 4 * B)
    print("%s: %d of %d candidate rows are tie-free" % (name, len(keep), 4 * B))
    assert len(keep) >= B


def test_table_reaches_every_path():
    named = set()
    for c in sc.CASES:
        for r in c.reaches:
            assert r in sc.REACH, (c.name, r)
            assert sc.REACH[r](c), "%s no longer reaches %s" % (c.name, r)
            named.add(r)
    assert named == set(sc.REACH), sorted(set(sc.REACH) - named)
    # every kind is in the table, and the batches cover one partial block and full 128-row blocks plus a ragged one
    assert {c.kind for c in sc.CASES} == set(sc.ORC)
    assert sc.BATCHES == (1, 37, 300) and 300 // 128 == 2 and 300 % 128


# ---- the batch axis ----------------------------------------------------------------------------------------
def test_ladder_reaches_every_path():
    """Every batch-dependent predicate of shape_cases is claimed by a (row, batch) that test_batch_sweep.py runs,
    and every claim holds at 256 CUs: an edit of a row or of a ladder value that loses a kernel fails here."""
    preds = dict(sc.FWD_PRED)
    preds.update(sc.BF16_PRED)
    preds.update(sc.BWD_PRED)
    assert len(preds) == len(sc.FWD_PRED) + len(sc.BF16_PRED) + len(sc.BWD_PRED)
    claimed = set()
    for row, B, names in sc.CLAIMS:
        c = sc.BY_NAME[row]
        for p in names.split():
            assert p in preds, (row, p)
            assert preds[p](c, B, sc.NCU), "%s at B = %d no longer reaches %s" % (row, B, p)
            if p in sc.FWD_PRED:
                assert B in sc.ladder(c), (row, B, p)
            elif p in sc.BF16_PRED:
                assert B in sc.BF16_LADDER and row in BF16_RUN, (row, B, p)
            else:
                assert (row, B) in sc.BWD_RUNS and not sc.backward_refused(c), (row, B, p)
            claimed.add(p)
    assert claimed == set(preds), sorted(set(preds) - claimed)
    # every ladder batch ends in a ragged 256-, 128- and 32-row block
    for B in sc.FWD_LADDER + sc.CIN_LADDER[:1] + sc.CIN_LADDER[3:] + (sc.B33K,):
        assert B % 256 and B % 128 and B % 32, B
    assert sc.FWD_LADDER[0] == sc.S3_COLS_MAX_B + 1 and sc.FWD_LADDER[2] > sc.WGRAD_SQ_ROWS and sc.FWD_LADDER[3] > 65536
    assert set(sc.BWD_KNOB_ROWS) | set(sc.BWD_LEFTOVER_ROWS) <= {r for r, B in sc.BWD_RUNS if B == sc.B33K}
    assert all(r in sc.BY_NAME for r, _ in sc.BWD_RUNS)
    # the slice_reduce4 leg of the knob cross-check changes the kernels launched: a float4 dW reduction with its
    # bias on one knob row, the head's two float4 passes on another
    assert any(sc.BWD_PRED["reduce_float4_bias"](sc.BY_NAME[r], sc.B33K, sc.NCU) for r in sc.BWD_KNOB_ROWS)
    assert any(sc.BWD_PRED["head_two_pass_float4"](sc.BY_NAME[r], sc.B33K, sc.NCU) for r in sc.BWD_KNOB_ROWS)
    # the accumulating per-chunk CIN dW (wgrad_s3 0) needs more than one chunk, the last one ragged
    c, B = sc.BY_NAME[sc.CIN_ACCUM_RUN[0]], sc.CIN_ACCUM_RUN[1]
    assert sc.CIN_ACCUM_RUN in sc.BWD_RUNS and sc.cin_rc_chunks(c, B) >= 2 and B * c.k % sc.cin_rc(c, B)


def test_batch_arithmetic():
    """The restated batch dispatch at the values the ladder's comments rely on."""
    assert [sc.s3_tile(B, 416, "dense") for B in sc.FWD_LADDER] == ["narrow2", "wave8", "dense16", "dense16"]
    assert [sc.s3_tile(B, 416, "k16") for B in sc.FWD_LADDER] == ["narrow2", "wave8", "mt2_gather", "mt2_gather"]
    assert [sc.s3_tile(B, 416, "any") for B in sc.FWD_LADDER] == ["narrow2", "wave8", "wave8", "wave8"]
    assert [sc.s3_tile(B, 832, "dense") for B in sc.FWD_LADDER] == ["narrow2", "dense16", "dense16", "dense16"]
    assert [sc.s3_tile(B, 208, "dense") for B in sc.FWD_LADDER] == ["narrow2", "narrow2", "wave8", "dense16"]
    assert sc.s3_tile(16256, 416, "dense") == "narrow2" and sc.s3_tile(16257, 416, "dense") == "wave8"
    assert sc.s3_tile(32512, 416, "dense") == "wave8" and sc.s3_tile(32513, 416, "dense") == "dense16"
    assert [sc.nt_tile(B, 512, "any") for B in (65535, 65536)] == ["small4", "large_even_v3"]
    assert sc.nt_tile(65573, 48, "dense") == "large_dense" and sc.nt_tile(65573, 112, "any") == "large_gather"
    c = sc.BY_NAME["xdeepfm_f5k16_33_cin200x7"]
    assert [sc.cin_tiles(c, B)[0][1] for B in sc.CIN_LADDER] == ["cin_2w", "cin_4w", "cin_8w", "cin_mt2", "cin_mt2"]
    assert [sc.cin_npad(h) for h in (5, 200, 208, 209, 256)] == [16, 208, 208, 256, 256]
    # head_train_kernel's grid: 33,000 rows reduce dW_out in one pass, 33,259 in two
    assert sc.head_blocks(33000) == (1000, 33) and sc.head_blocks(sc.B33K) == (1008, 33) and 1008 % 16 == 0
    assert sc.head_blocks(65536) == (1024, 64) and sc.head_blocks(65573) == (1009, 65)
    # the CIN backward's chunk: 64 M floats over rows of 4,368 (F Hp = 4,352 padded to 21 x 208)
    c = sc.BY_NAME["xdeepfm_f17k16_500x7_cin256x3"]
    assert sc.cin_rc(c, 1024) == 15360 and sc.cin_rc_chunks(c, 1024) == 2 and 1024 * 16 - 15360 == 1024
    assert sc.cin_rc_chunks(sc.BY_NAME["xdeepfm_f5k16_100x37_cin10x7"], 4099) == 1
    assert sc.wgrad_s3_slices(16400, 37, 20) == (256, 96) and 16400 % 96
    # where the dW, the bias gradient and dW_out land in mats: whole float4s reduce as float4s only from a 16-byte
    # boundary.  37 x 400: layer 2's W at 20 37 + 37 = 777, its bias at 15,577, W_out at 15,977 -- all scalar
    assert [w[3:] for w in sc.wgrads(sc.BY_NAME["dnn_f5k4_37x400"])] == [(0, 740), (777, 15577)]
    assert sc.linears(sc.BY_NAME["dnn_f5k4_37x400"])[1] == (15977, 400)
    assert [sc.reduce_float4(*w) for w in sc.wgrads(sc.BY_NAME["dnn_f5k4_37x400"])] == [False, False]
    assert not sc.head_float4(sc.BY_NAME["dnn_f5k4_37x400"])
    offsets = [w[3:] for w in sc.wgrads(sc.BY_NAME["dnn_f9k16_24x8x200x7x16"])]
    assert offsets[:3] == [(0, 3456), (3480, 3672), (3680, 5280)]
    assert [sc.reduce_float4(*w) for w in sc.wgrads(sc.BY_NAME["dnn_f9k16_24x8x200x7x16"])] == [True, True, True, False,
                                                                                                False]
    assert sc.head_float4(sc.BY_NAME["pnn_f7k10_33x20"]) and not sc.head_float4(sc.BY_NAME["deepfm_f13k16_209x37"])
    # W^T planes: 200 -> 7 (K = 200 within 16 of 208, its input 224 wide), 413 -> 401; none over K = 20
    assert [L.NTpad for L in sc.tower_layers(sc.BY_NAME["dnn_f9k16_24x8x200x7x16"])] == [0, 0, 0, 208, 0]
    assert [L.NTpad for L in sc.tower_layers(sc.BY_NAME["dnn_f5k4_413x401"])] == [0, 416]
    assert [L.NTpad for L in sc.tower_layers(sc.BY_NAME["deepfm_f13k16_209x37"])] == [208, 0]
    assert [L.Npad for L in sc.tower_layers(sc.BY_NAME["deepfm_f13k16_209x37"])] == [224, 48]


def test_wgrad_slices_restated():
    """shape_cases.wgrad_sq_slices is train.hip's wgrad_sq_slices (a host function: no GPU), at the shapes of the
    backward runs, at the bench's pinned ones (test_abi.py) and at other CU counts."""
    from rmx import _lib
    S = _lib.lib.rmx_debug_wgrad_slices
    shapes = {(B, N, K) for r, B in sc.BWD_RUNS if sc.wgrad_sq(B) for N, K, *_ in sc.wgrads(sc.BY_NAME[r])}
    shapes |= {(65536, 400, 624), (65536, 400, 400), (32768, 1, 1), (1 << 20, 832, 624)}
    assert len(shapes) > 12
    for rows, N, K in sorted(shapes):
        for ncu in (256, 304, 64):
            assert S(rows, N, K, ncu) == sc.wgrad_sq_slices(rows, N, K, ncu), (rows, N, K, ncu)
    assert sc.wgrad_sq_slices(65536, 400, 624) == 40


@pytest.mark.parametrize("name,B", sc.BWD_RUNS)
def test_backward_tie_rule_ladder(name, B):
    keep = sc.tie_free_rows(name, 4 * B)
    print("%s B=%d: %d of %d candidate rows are tie-free" % (name, B, len(keep), 4 * B))
    assert len(keep) >= B


def tail_rows(name, B):
    """The rows a backward kernel's last partial 32-row chunk holds; for a CIN backward in more than one chunk of
    B k rows, the samples of the last chunk (at the default knobs that chunk feeds mats only through the layers
    below the top CIN layer, whose dL/du it carries; with wgrad_s3 0 every CIN dW is summed chunk by chunk)."""
    c = sc.BY_NAME[name]
    if sc.cin_rc_chunks(c, B) >= 2:
        return (B * c.k % sc.cin_rc(c, B)) // c.k
    return B % 32


@pytest.mark.parametrize("name,B", sc.BWD_RUNS)
def test_tail_sensitivity(name, B):
    """Leaving the last partial chunk out of the batch sums moves the mats gradient past grad_check._close's bars
    -- a kernel that drops its ragged tail cannot pass test_batch_sweep.py's backward.  (The last 8 rows alone:
    measured and printed.)  Figures in DESIGN.md §4.  xdeepfm_f5k16_100x37_cin10x7 at 2,048 has no partial chunk
    (B % 32 == 0, one CIN chunk): nothing is asserted for it here, the same row at 4,099 carries the assertion; 2,048
    is in the list for the CIN's dL/dz split GEMM on the 8-wave tile (M = 32,768 rows; claim cin_dz_wave8)."""
    from grad_check import _close
    ref = sc.oracle_backward(name, B)["mats"].astype(np.float64)
    n = tail_rows(name, B)
    for rows in (n, 8):
        if rows == 0:
            continue
        move = sc.oracle_mats_share(name, B, rows)
        rel, elem = sc.close_bars(move, ref)
        print("%s B=%d: without the last %d rows the mats gradient moves by %.3g x the array bar, %.3g x the "
              "element-wise bar" % (name, B, rows, rel, elem))
        if rows == n:
            assert not _close(ref - move, ref), (name, B, rows, rel, elem)
    if n == 0:  # B % 32 == 0 and one CIN chunk: no partial chunk to drop
        assert B % 32 == 0


def test_shape_arithmetic():
    """The restated dispatch at the values the table's comments rely on."""
    assert [sc.needs_gather_x(k) for k in (1, 4, 8, 10, 16)] == [True, False, False, True, False]
    assert [sc.needs_gather_x(k, True) for k in (1, 4, 8, 10, 16)] == [True, True, False, True, False]
    assert [(F + 15) // 16 for F in (16, 17, 32, 33, 48, 49, 64)] == [1, 2, 2, 3, 3, 4, 4]
    # 400 -> two 208-column slices, 832 -> four; 200 pads to 224 (seven tiles twice), never to one 208 block
    assert [sc.tower_npad(n) for n in (400, 832, 817, 200, 208, 500, 520, 7, 37)] == [416, 832, 832, 224, 224, 512,
                                                                                      544, 16, 48]
    assert [sc.tower_npad(n) % 208 for n in (400, 832, 200, 500)] == [0, 0, 16, 96]
    assert [sc.tower_nt(sc.tower_npad(n)) for n in (400, 832, 200, 500, 520)] == [26, 26, 7, 16, 2]
    assert [sc.one_block(n) for n in (400, 416, 417, 520, 832, 200)] == [True, True, False, False, False, False]
    # DCN F = 64: depth 15 asks for exactly 64 KB of LDS, depth 16 for more
    c15, c16 = sc.BY_NAME["dcn_f64k16_16_d15"], sc.BY_NAME["dcn_f64k16_16_d16"]
    assert sc.cross_lds(c15) == 64 * 1024 and sc.cross_lds(c16) == 68 * 1024
