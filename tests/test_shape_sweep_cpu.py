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
edited away from it."""
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
