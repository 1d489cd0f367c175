"""The shapes of the off-benchmark sweep (test_shape_sweep_cpu.py, test_shape_sweep.py): every model kind away
from F = 39 / k = 16 / towers off the tuned widths, with the helpers that build the rmx model, the oracle model,
the table, the ids and the references of a row.  V = 5,003, the seeds of test_gpu_parity.py, initMats weights
(orc_init_mats: the same bits as rmx_model_init_mats, test_abi.py) and bias 0.01.

A row names what it is there for in `reaches`; REACH holds, per name, the shape arithmetic (the dispatch of
csrc/models.hip, k_gemm.hip and k_interact.hip restated in Python) that must hold for a row that claims it, so
an edit of the table that loses a path fails test_shape_sweep_cpu.py::test_table_reaches_every_path.

"The batch axis" further down does the same for the kernels that the batch picks: the ladders of batches and the
(row, batch) backward runs of test_batch_sweep.py, the batch-dependent dispatch restated as predicates of
(row, batch, CU count), and CLAIMS (test_shape_sweep_cpu.py::test_ladder_reaches_every_path)."""
import collections
import functools

import numpy as np

import oracle_ctypes as oc

V = 5003
SEED_IDS, SEED_TAB, SEED_MATS = 0x5EED2026, 0x7AB1E, 0x3A75
BIAS = 0.01
TOL, TOL_BF16 = 1e-5, 2e-4
BATCHES = (1, 37, 300)
LARGE_B = 65536
LARGE_NAMES = ("dnn_f17k8_400x400x400", "dcn_f17k8_400x400x400_d3")  # also run at LARGE_B, fp32 and bf16
ORC = {"lr": oc.LR, "deepfm": oc.DEEPFM, "dnn": oc.DNN, "dcn": oc.DCN, "pnn": oc.PNN, "xdeepfm": oc.XDEEPFM}

Case = collections.namedtuple("Case", "name kind F k fc cin cross reaches bf16 edge16 scale row0 mseed")

# ---- the dispatch arithmetic, restated -------------------------------------------------------------------
K_NTS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16, 20, 25, 26)  # k_gemm.hpp kNTs
MAX_FUSED_CROSS = 8                                        # rmx_models.hpp kMaxFusedCross
ROW_OWNER_MAX_F = 40                                       # kFmMaxF, kGMaxF, kSMaxF


def tower_npad(N):
    """k_gemm.hip tower_npad_for at the default knobs."""
    nt = (N + 15) // 16
    even = nt >= 8
    best, best_pad = -1, 1 << 30
    for c in K_NTS:
        if even and c % 2:
            continue
        pad = (nt + c - 1) // c * c
        if pad < best_pad or (pad == best_pad and c > best):
            best_pad, best = pad, c
    return best_pad * 16


def tower_nt(npad):
    """k_gemm.hip tower_nt_for: the column tiles of one block."""
    return max(c for c in K_NTS if (npad // 16) % c == 0)


def one_block(N):
    """the layer's columns fit one GEMM block (an output layer that does not goes through tower_head_kernel
    in fp32 and is refused in bf16)"""
    return tower_nt(tower_npad(N)) * 16 == tower_npad(N)


def needs_gather_x(k, bf16=False):
    """models.hip needs_gather_x: the GEMM gathers 16-B slots from table rows, else x is materialised."""
    return k % (8 if bf16 else 4) != 0


def dcn_fused(c):
    return c.kind == "dcn" and len(c.fc) >= 2 and c.cross <= MAX_FUSED_CROSS


def cross_lds(c):
    return 4 * (c.cross + 1) * c.F * 16


def cross16_fmax(c):
    """k_interact.hip launch_cross by ids: the cross16_kernel instantiation, or 0 for the generic kernel."""
    if dcn_fused(c) or c.k != 16 or c.F > 64 or cross_lds(c) > 64 * 1024:
        return 0
    return 16 if c.F <= 16 else (40 if c.F <= 40 else 64)


def product_ntile(c):
    """k_interact.hip launch_product by ids: product16_kernel's NTILE, or 0 for the generic kernel."""
    return (c.F + 15) // 16 if c.kind == "pnn" and c.k == 16 and c.F <= 64 else 0


def encoder_fm_x(c):
    """models.hip: DeepFM fp32 at B <= 2,048 with k = 16 and two or more layers runs column-split -- the
    encoder stores x (stage encoder_fm_x) and every layer reads dense A.  (The sweep's batches are all below
    2,048: no row-owner kernel, tower_small or tower_fused, runs at the defaults.)"""
    return c.kind == "deepfm" and c.k == 16 and len(c.fc) >= 2


def bf16_refused(c):
    return c.kind != "lr" and not one_block(c.fc[-1])


def hidden(c):
    """widths of the layers that are not the last hidden one (they run the ReLU-store epilogue)"""
    return c.fc[:-1]


REACH = {
    # layer 1 from the table
    "gather_any_fp32": lambda c: c.kind != "pnn" and c.k != 16 and c.k % 4 == 0,
    "gather_any_bf16": lambda c: c.kind != "pnn" and c.bf16 and c.k != 16 and c.k % 8 == 0,
    "gather_x_fp32": lambda c: c.kind != "pnn" and needs_gather_x(c.k),
    "gather_x_bf16": lambda c: c.kind != "pnn" and c.bf16 and needs_gather_x(c.k, True),
    "encoder_generic": lambda c: c.kind in ("deepfm", "dcn", "pnn") and c.k != 16,
    "k_1": lambda c: c.k == 1,
    "F_1": lambda c: c.F == 1 and c.kind != "lr",
    # tower widths
    "N_not_multiple_of_16": lambda c: any(n % 16 for n in c.fc),
    "N_odd": lambda c: any(n % 2 for n in c.fc),
    "N_1_to_7": lambda c: any(n < 8 for n in c.fc),
    "hidden_over_416": lambda c: any(n > 416 and tower_nt(tower_npad(n)) in (10, 16, 20) for n in hidden(c)),
    "split_4_slices_hidden": lambda c: any(tower_npad(n) == 832 for n in hidden(c)),
    "npad_224_hidden": lambda c: any(193 <= n <= 208 and tower_npad(n) % 208 != 0 for n in c.fc),
    "last_hidden_832": lambda c: c.fc[-1] > 816 and tower_npad(c.fc[-1]) == 832 and not one_block(c.fc[-1]),
    "tower_head_kernel": lambda c: not one_block(c.fc[-1]),
    "bf16_refused": lambda c: c.bf16 and bf16_refused(c),
    "five_layers": lambda c: len(c.fc) >= 5,
    # dense A on the split GEMM with K % 4 != 0: the last 16-byte slot of a row runs past K.  Forward: a layer of
    # Npad % 208 == 0 over a layer of odd width; backward dX: a layer with W^T planes (its K within 16 of a
    # multiple of 208) and an odd width N, the K of that GEMM; the CIN's dL/dz: K = the layer's maps
    "split_forward_K_tail": lambda c: any(c.fc[i - 1] % 4 and tower_npad(c.fc[i]) % 208 == 0 for i in range(1, len(c.fc))),
    "split_dx_K_tail": lambda c: any(c.fc[i] % 4 and -c.fc[i - 1] % 208 <= 16 + (-c.fc[i - 1] % 16)
                                     for i in range(1, len(c.fc))),
    # DeepFM around the F limit of the row-owner kernels and of the FM fused into layer 1
    "F_40": lambda c: c.kind == "deepfm" and c.F == ROW_OWNER_MAX_F and c.k == 16,
    "F_41": lambda c: c.kind == "deepfm" and c.F == ROW_OWNER_MAX_F + 1 and c.k == 16,
    # PNN
    "product_generic": lambda c: c.kind == "pnn" and product_ntile(c) == 0,
    "product16_ntile1": lambda c: product_ntile(c) == 1,
    "product16_ntile2": lambda c: product_ntile(c) == 2,
    "product16_ntile3": lambda c: product_ntile(c) == 3,
    "product16_ntile4": lambda c: product_ntile(c) == 4,
    "product16_tile_edge": lambda c: product_ntile(c) > 0 and (c.F % 16 == 0 or c.F % 16 == 1),
    # DCN
    "cross_fused_F_edge": lambda c: dcn_fused(c) and c.k == 16 and c.F in (16, 17, 40, 41, 64),
    "cross_fused_F_over_40": lambda c: dcn_fused(c) and c.F > ROW_OWNER_MAX_F,
    "cross16_16": lambda c: c.kind == "dcn" and cross16_fmax(c) == 16,
    "cross16_40": lambda c: c.kind == "dcn" and cross16_fmax(c) == 40,
    "cross16_64": lambda c: c.kind == "dcn" and cross16_fmax(c) == 64,
    "cross_generic": lambda c: c.kind == "dcn" and not dcn_fused(c) and cross16_fmax(c) == 0,
    "cross_generic_k_not_16": lambda c: c.kind == "dcn" and not dcn_fused(c) and c.k != 16,
    "cross_lds_exactly_64k": lambda c: c.kind == "dcn" and cross16_fmax(c) == 64 and cross_lds(c) == 64 * 1024,
    "cross_lds_fall_through": lambda c: c.kind == "dcn" and c.k == 16 and c.F <= 64 and not dcn_fused(c) and
    cross_lds(c) > 64 * 1024,
    "cross_unfused_depth": lambda c: c.kind == "dcn" and c.cross > MAX_FUSED_CROSS,
    # xDeepFM
    "cin_maps_not_multiple_of_4": lambda c: c.kind == "xdeepfm" and len(c.cin) > 1 and c.cin[0] % 4 != 0,
    "cin_dz_K_tail": lambda c: c.kind == "xdeepfm" and any(h % 4 for h in c.cin),
    "cin_F_over_40": lambda c: c.kind == "xdeepfm" and c.F > ROW_OWNER_MAX_F,
    "cin_256": lambda c: c.kind == "xdeepfm" and max(c.cin) == 256,
    # M >= 65,536 picks other tiles, with exclusions of their own for a layer 1 gathered at k != 16
    "large_batch_gather_any": lambda c: c.name in LARGE_NAMES and c.k != 16 and c.k % 8 == 0 and c.fc[0] == 400,
    # rows of the batch ladder (below): what their shapes alone must keep true
    "split_layer_odd_width": lambda c: any(n % 2 and tower_npad(n) % 208 == 0 for n in c.fc),
    "fm_fusable_F_not_39": lambda c: c.kind == "deepfm" and c.k == 16 and c.F not in (39, 40, 41) and
    c.F <= ROW_OWNER_MAX_F and len(c.fc) >= 2 and c.fc[0] != 400 and tower_npad(c.fc[0]) % 208 == 0,
    "emb_fused_F_not_39": lambda c: c.kind == "deepfm" and c.k == 16 and c.F != 39 and c.F * 16 % 208 == 0,
    "wgrad_sq_one_column_tile": lambda c: any(n % 208 == 1 for n in c.fc),
    "cin_split": lambda c: c.kind == "xdeepfm" and any(cin_npad(h) == 208 for h in c.cin),
    # LR
    "lr_F_1": lambda c: c.kind == "lr" and c.F == 1,
    "lr_F_65": lambda c: c.kind == "lr" and c.F == 65,
}


# What test_shape_sweep_cpu.py's conditions ask of a row beyond the defaults, found by measuring the oracle:
#   scale   power of two on the output weights over the last hidden layer, so that a layer's edge moves p by
#           10 TOL (DCN: the cross term carries most of the logit; wide last layers: one unit of 832 is small);
#   mseed   initMats seed offset, where the default seed leaves the last unit of a narrow layer dead on every
#           row (ReLU 0: no scale makes it visible), or nearly so: deepfm_f13k16_209x37 shows its weakest edge
#           (layer 2's last unit) at 1.7e-4 on seed offset 0, where no scale reaches 8e-4 in bf16 with the
#           emulation within 1e-4 of f64 (scale 4: 6.9e-4 / 1.2e-4), and at 1.1e-3 / 3.1e-5 on offset 1, scale 1
#           (offsets 2, 3, 4 at scale 1: 9.2e-4, 1.4e-3, 1.1e-3, all within the error bar too);
#   edge16  False: the row runs in bf16 at the bf16 bar, but its weakest edge (PNN: the last pair's column of the
#           product block) stays below 4 TOL_BF16 at any scale that keeps the bf16 emulation within TOL_BF16 / 2
#           of f64 -- the fp32 run is that edge's check.
# Measured for the edge16 False rows (oracle, B = 128; both grow linearly with the scale, so no scale separates
# them): the first power-of-two scale at which the weakest edge reaches 4 TOL_BF16 = 8e-4 in the bf16 emulation,
# and max |p(bf16 emulation) - p(f64)| there, which must stay <= TOL_BF16 / 2 = 1e-4 (mats seeds 0 .. 4 were
# tried as well; at the scale kept in the table every row has that error <= 6.9e-5):
#   pnn_f17k8_500x7          scale  8: edge 1.2e-3, error 2.6e-4   (scale 4: 5.9e-4, 1.3e-4)
#   dnn_f9k16_24x8x200x7x16  scale 64: edge 1.6e-3, error 5.5e-4   (scale 32: 7.9e-4, 2.7e-4)
#   pnn_f16k16_48x32         scale  4: edge 8.2e-4, error 1.02e-4  (scale 2: 4.1e-4, 5.1e-5)
#   pnn_f17k16_48x32         scale  4: edge 1.1e-3, error 1.2e-4
#   pnn_f32k16_48x32         scale  4: edge 1.1e-3, error 1.4e-4
#   pnn_f33k16_48x32         scale  8: edge 1.2e-3, error 2.5e-4
#   pnn_f48k16_48x32         scale  8: edge 9.3e-4, error 3.0e-4
#   pnn_f49k16_48x32         scale  8: edge 1.1e-3, error 4.0e-4
#   pnn_f64k16_48x32         scale 32: edge 1.4e-3, error 8.0e-4
#   pnn_f65k16_48x32         scale  4: edge 8.8e-4, error 2.5e-4
TUNED = {
    "dcn_f7k10_33x20_d3": dict(scale=4), "pnn_f7k10_33x20": dict(scale=4, mseed=1),
    "deepfm_f2k1_5x3": dict(scale=4, mseed=1), "pnn_f17k8_500x7": dict(edge16=False),
    "deepfm_f39k16_200x832": dict(scale=2), "dnn_f39k16_200x832": dict(scale=2),
    "dnn_f9k16_24x8x200x7x16": dict(scale=8, mseed=1, edge16=False),
    "deepfm_f40k16_400x400x400": dict(scale=2), "deepfm_f41k16_400x400x400": dict(scale=2),
    "pnn_f16k16_48x32": dict(edge16=False), "pnn_f17k16_48x32": dict(edge16=False),
    "pnn_f32k16_48x32": dict(edge16=False), "pnn_f33k16_48x32": dict(edge16=False),
    "pnn_f48k16_48x32": dict(edge16=False), "pnn_f49k16_48x32": dict(edge16=False),
    "pnn_f64k16_48x32": dict(scale=2, mseed=1, edge16=False), "pnn_f65k16_48x32": dict(mseed=4, edge16=False),
    "dcn_f16k16_64x32_d3": dict(scale=2), "dcn_f17k16_64x32_d3": dict(scale=2), "dcn_f40k16_64x32_d3": dict(scale=8),
    "dcn_f41k16_64x32_d3": dict(scale=4), "dcn_f64k16_64x32_d3": dict(scale=8, mseed=1),
    "dcn_f16k16_32_d3": dict(scale=2), "dcn_f17k16_32_d3": dict(scale=4), "dcn_f40k16_32_d3": dict(scale=4),
    "dcn_f41k16_32_d3": dict(scale=2), "dcn_f16k16_48x24_d9": dict(scale=2), "dcn_f64k16_16_d15": dict(scale=16),
    "dcn_f64k16_16_d16": dict(scale=8), "dnn_f17k8_400x400x400": dict(scale=4, mseed=3),
    "dcn_f17k8_400x400x400_d3": dict(scale=4), "dnn_f5k4_37x400": dict(scale=8),
    "dnn_f5k4_413x401": dict(scale=4), "deepfm_f13k16_209x37": dict(mseed=1),
}


def _c(kind, F, k, fc, reaches, cin=(), cross=0, bf16=None, row0=3):
    name = "%s_f%dk%d" % (kind, F, k)
    if fc:
        name += "_" + "x".join(str(d) for d in fc)
    if cin:
        name += "_cin" + "x".join(str(d) for d in cin)
    if cross:
        name += "_d%d" % cross
    if bf16 is None:
        bf16 = kind != "xdeepfm"  # the CIN has no bf16 path
    t = TUNED.get(name, {})
    return Case(name, kind, F, k, tuple(fc), tuple(cin), cross, tuple(reaches.split()), bf16,
                bf16 and t.get("edge16", True), t.get("scale", 1), row0, SEED_MATS + t.get("mseed", 0))


def _rows():
    r = []
    for kind in ("deepfm", "dnn", "dcn"):
        r.append(_c(kind, 5, 4, (100, 37), "gather_any_fp32 gather_x_bf16 N_not_multiple_of_16 N_odd" +
                    (" encoder_generic" if kind != "dnn" else ""), cross=2 if kind == "dcn" else 0))
    for kind in ("deepfm", "dnn", "pnn"):
        r.append(_c(kind, 17, 8, (500, 7), "hidden_over_416 N_1_to_7 N_odd" +
                    (" gather_any_fp32 gather_any_bf16" if kind != "pnn" else " product_generic encoder_generic")))
    for kind in ("deepfm", "dnn", "dcn", "pnn"):
        r.append(_c(kind, 7, 10, (33, 20), "N_odd N_not_multiple_of_16" +
                    (" gather_x_fp32 gather_x_bf16" if kind != "pnn" else " product_generic") +
                    (" encoder_generic" if kind != "dnn" else ""), cross=3 if kind == "dcn" else 0))
    r.append(_c("deepfm", 2, 1, (5, 3), "k_1 gather_x_fp32 gather_x_bf16 N_1_to_7"))
    r.append(_c("deepfm", 1, 16, (16,), "F_1"))
    for kind in ("deepfm", "dnn"):
        r.append(_c(kind, 3, 32, (520,), "tower_head_kernel bf16_refused gather_any_fp32 gather_any_bf16"))
        r.append(_c(kind, 39, 16, (832, 200), "split_4_slices_hidden npad_224_hidden tower_head_kernel bf16_refused"))
        r.append(_c(kind, 39, 16, (200, 832), "last_hidden_832 tower_head_kernel bf16_refused npad_224_hidden"))
    r.append(_c("dnn", 9, 16, (24, 8, 200, 7, 16), "five_layers N_1_to_7 split_dx_K_tail"))
    r.append(_c("dnn", 5, 4, (37, 400), "split_forward_K_tail"))
    r.append(_c("deepfm", 40, 16, (400, 400, 400), "F_40"))
    r.append(_c("deepfm", 41, 16, (400, 400, 400), "F_41"))
    r.append(_c("pnn", 2, 4, (7,), "product_generic N_1_to_7"))
    for F in (16, 17, 32, 33, 48, 49, 64, 65):
        nt = (F + 15) // 16
        r.append(_c("pnn", F, 16, (48, 32), "product_generic" if F > 64 else "product16_ntile%d product16_tile_edge" % nt))
    for F in (16, 17, 40, 41, 64):  # the cross stack rides tower layer 1 (two layers, depth <= 8)
        r.append(_c("dcn", F, 16, (64, 32), "cross_fused_F_edge" + (" cross_fused_F_over_40" if F > 40 else ""), cross=3))
    for F, fm in ((16, 16), (17, 40), (40, 40), (41, 64)):  # one layer: the cross stack runs its own kernel
        r.append(_c("dcn", F, 16, (32,), "cross16_%d" % fm, cross=3))
    # ... and off k = 16 the generic cross kernel (f = d / k, the d < D lane guard): k % 4 != 0 and k = 8
    r.append(_c("dcn", 7, 10, (33,), "cross_generic_k_not_16 cross_generic gather_x_fp32 encoder_generic", cross=3))
    r.append(_c("dcn", 17, 8, (32,), "cross_generic_k_not_16 cross_generic gather_any_fp32 encoder_generic", cross=3))
    r.append(_c("dcn", 16, 16, (48, 24), "cross_unfused_depth cross16_16", cross=9))
    r.append(_c("dcn", 64, 16, (16,), "cross_lds_exactly_64k cross16_64 cross_unfused_depth", cross=15))
    r.append(_c("dcn", 64, 16, (16,), "cross_lds_fall_through cross_generic cross_unfused_depth", cross=16))
    r.append(_c("xdeepfm", 5, 16, (100, 37), "cin_maps_not_multiple_of_4 cin_dz_K_tail N_odd", cin=(10, 7)))
    r.append(_c("xdeepfm", 41, 16, (33,), "cin_F_over_40 N_odd", cin=(5,)))
    r.append(_c("xdeepfm", 17, 16, (500, 7), "cin_256 hidden_over_416", cin=(256, 3)))
    # layer 1 gathered at k = 8 into the 400-wide tiles: at B = 65,536 the large-batch tile variants (LARGE_B)
    r.append(_c("dnn", 17, 8, (400, 400, 400), "large_batch_gather_any"))
    r.append(_c("dcn", 17, 8, (400, 400, 400), "large_batch_gather_any encoder_generic", cross=3))
    # rows of the batch ladder (FWD_LADDER / CIN_LADDER / BWD_RUNS below): split-GEMM layers of odd width, the second
    # over K = 413; DeepFM with the FM fused into a gathered split-GEMM layer 1 and the embedding gradient in the
    # layer-1 dX epilogue away from F = 39 (F 16 = 208, 416); a 209-wide layer (the 208 x 208 dW's second N tile
    # holds one column); a CIN layer of 200 maps, the only width that runs the split CIN tiles
    r.append(_c("dnn", 5, 4, (413, 401), "split_layer_odd_width split_forward_K_tail split_dx_K_tail gather_any_fp32"))
    r.append(_c("deepfm", 13, 16, (401, 37), "fm_fusable_F_not_39 emb_fused_F_not_39 split_layer_odd_width"))
    r.append(_c("deepfm", 26, 16, (413, 20), "fm_fusable_F_not_39 emb_fused_F_not_39 split_layer_odd_width"))
    r.append(_c("deepfm", 13, 16, (209, 37), "wgrad_sq_one_column_tile emb_fused_F_not_39"))
    r.append(_c("xdeepfm", 5, 16, (33,), "cin_split cin_dz_K_tail", cin=(200, 7)))
    r.append(_c("lr", 1, 16, (), "lr_F_1"))
    r.append(_c("lr", 65, 16, (), "lr_F_65"))
    return r


CASES = _rows()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and set(TUNED) <= set(BY_NAME)
NAMES = [c.name for c in CASES]
BF16_NAMES = [c.name for c in CASES if c.bf16]


def backward_refused(c):
    """train.hip: the cross backward is the closed form, at most kMaxFusedCross layers deep."""
    return c.kind == "dcn" and c.cross > MAX_FUSED_CROSS


# ---- the batch axis ----------------------------------------------------------------------------------------
# The batch picks the kernel as much as the shape does.  Below: the batch-dependent dispatch of k_gemm_s3.hip
# (launch_tower_s3, launch_cin_s3), k_gemm.hpp (launch_tower_nt, launch_cin_nt), models.hip (model_forward) and
# train.hip (wgrad, model_train) restated at the default knobs as predicates of (case, batch, CU count); the
# ladders of batches test_batch_sweep.py runs; and CLAIMS, which names a (row, batch) for every predicate.
# test_shape_sweep_cpu.py::test_ladder_reaches_every_path evaluates every claim at 256 CUs.
#
# No ladder value is a multiple of 32, 128 or 256: every batch ends in a ragged block and a ragged 32-row chunk.
#   2,049   one row past s3_cols = 2,048 (DeepFM leaves the column-split path); every split layer on 2-wave tiles
#   16,400  ceil(B / 128) * 2 = 258 >= 256: the 8-wave MT = 1 tile on a 416-wide layer (and the staggered / 16-wave
#           tiles on an 832-wide one: ceil(B / 256) * 4 = 260)
#   33,259  > 32,768: the 208 x 208 dW; ceil(B / 256) * 2 = 260 >= 256: the 16-wave dense and the MT = 2 gather
#           tiles on a 416-wide layer.  Not 33,000: head_train_kernel splits B into np = ceil(B / ceil(B / 1024))
#           blocks and reduces dW_out in two passes only when np % 16 == 0; 33,000 gives np = 1,000 (one pass),
#           33,232 .. 33,264 give np = 1,008.  33,259 % 32 = 11, % 128 = 107, % 256 = 235
#   65,573  >= 65,536: the fp32 / bf16 MFMA engine's large-batch tiles; ceil(B / 256) = 257 >= 256: the dX split
#           GEMM of a 208-wide layer on the blocks2 >= 256 tiles
# CIN rows (M = 16 B rows per launch): 509 (M = 8,144 < 8,192, ceil(M / 64) = 128 < 256: 2-wave), 1,024 (4-wave),
# 2,048 (8-wave), 4,099 (ceil(M / 256) = 257: MT = 2), 16,400
NCU = 256
FWD_LADDER = (2049, 16400, 33259, 65573)
CIN_LADDER = (509, 1024, 2048, 4099, 16400)
BF16_LADDER = (16400, 65573)
B33K = 33259
S3_COLS_MAX_B = 2048       # rmx_internal.hpp kS3ColsMaxB
WGRAD_SQ_ROWS = 32768      # train.hip wgrad: rows >= this take the 208 x 208 tile
HEAD_MAX_N = 512           # train.hip kHeadCols * 64
K_CIN_NTS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16)  # k_gemm.hpp kCinNTs

Lay = collections.namedtuple("Lay", "K N Neff Npad amode NTpad ldin blocks bias_fusable")


def ladder(c):
    return CIN_LADDER if c.kind == "xdeepfm" else FWD_LADDER


def _up(n, m):
    return (n + m - 1) // m * m


def cin_npad(H):
    """k_gemm.hip cin_npad_for"""
    return min(c for c in K_CIN_NTS if c >= (H + 15) // 16) * 16


def tower_layers(c, bf16=False):
    """The tower's Linears as models.hip builds them: K, N with the fused DCN's extra columns, the layer's own
    width Neff, Npad, how the forward by ids forms A (k16 / any: gathered from the table, dense), NTpad of the
    W^T planes (0: none, alloc_wt), the row stride of its input in the backward, the K blocks of its dW (PNN's
    layer 1: two) and whether its bias gradient can ride the dW (bias_mode 1)."""
    D, P = c.F * c.k, c.F * (c.F - 1) // 2
    out, prev, ld = [], D, _up(D, 16)
    for i, d in enumerate(c.fc):
        K, N, blocks = prev, d, (prev,)
        if i == 0 and c.kind == "pnn":
            K, blocks = D + P, (D, P)
            ld = _up(K, 16)
        if i == 0 and dcn_fused(c):
            N = d + c.cross + 1
        amode = "dense"
        if i == 0 and c.kind != "pnn" and not needs_gather_x(c.k, bf16):
            amode = "k16" if c.k == 16 else "any"
        wt = len(blocks) == 1 and N == d and _up(K, 208) - _up(K, 16) <= 16
        out.append(Lay(K, N, d, tower_npad(N), amode, _up(K, 208) if wt else 0, ld, blocks,
                       not (i == 0 and c.kind == "pnn")))
        prev, ld = d, tower_npad(N)
    return out


def row_owner_candidate(c, i, L):
    """A layer the row-owner kernels (tower_small / tower_fused / head / tail / layer_s3: 400-wide layers only)
    may take at some batch: the tile predicates leave it alone."""
    return L.Neff == 400 and (L.K == 400 or (i == 0 and c.kind == "deepfm" and c.k == 16))


def s3_blocks2(M, npad):
    return (M + 255) // 256 * (npad // 208)


def s3_tile(M, npad, amode, ncu=NCU, ids=True):
    """k_gemm_s3.hip launch_tower_s3 at the default knobs (no cols32)."""
    mt2 = (amode == "dense" or (amode == "k16" and ids)) and s3_blocks2(M, npad) >= 256
    if not mt2 and (M + 127) // 128 * (npad // 208) < ncu:
        return "narrow2"
    if mt2:
        return "dense16" if amode == "dense" else "mt2_gather"
    return "wave8"


def nt_tile(M, npad, amode):
    """k_gemm.hpp launch_tower_nt / tower_variant_for (fp32 and bf16 alike but for the 26-tile variants)."""
    nt = tower_nt(npad)
    if M < 65536:
        return "small4"
    if nt == 26:
        return "large_nt26"
    if nt % 2 == 0 and nt >= 8:
        return "large_even_v3"
    return "large_dense" if amode == "dense" else "large_gather"


def cols32_path(c, B):
    """models.hip: DeepFM fp32, k = 16, two or more layers, B <= s3_cols."""
    return encoder_fm_x(c) and B <= S3_COLS_MAX_B


def fwd_tiles(c, B, ncu=NCU, bf16=False):
    """[(layer, engine, tile)] of forward_ids: the layers the per-layer path runs on the split GEMM ("s3"), the
    fp32 MFMA engine ("f32") or the bf16 one, row-owner candidates and the column-split path left out."""
    if c.kind == "lr" or (not bf16 and cols32_path(c, B)):
        return []
    out = []
    for i, L in enumerate(tower_layers(c, bf16)):
        if row_owner_candidate(c, i, L) or (bf16 and L.Npad == 416 and i > 0):  # (bf16: tower_tail pairs)
            continue
        if bf16:
            out.append((i, "bf16", nt_tile(B, L.Npad, L.amode)))
        elif L.Npad % 208 == 0:
            out.append((i, "s3", s3_tile(B, L.Npad, L.amode, ncu)))
        else:
            out.append((i, "f32", nt_tile(B, L.Npad, L.amode)))
    return out


def _has(c, B, ncu, engine, tile, bf16=False):
    return any(e == engine and t == tile for _, e, t in fwd_tiles(c, B, ncu, bf16))


def cin_tiles(c, B, ncu=NCU):
    """[(layer, tile)]: launch_cin_s3 (Npad == 208) by M = B k against the CU count, launch_cin_nt by M."""
    out, M = [], B * c.k
    for i, h in enumerate(c.cin if c.kind == "xdeepfm" else ()):
        if cin_npad(h) == 208:
            blocks = lambda rows: (M + rows - 1) // rows
            t = "cin_mt2" if blocks(256) >= ncu else "cin_8w" if blocks(128) >= ncu else \
                "cin_4w" if blocks(64) >= ncu else "cin_2w"
        else:
            t = "cin_f32_lt_8192" if M < 8192 else "cin_f32_ge_8192"
        out.append((i, t))
    return out


def deepfm_fm_fused_layer1(c, B):
    """models.hip fm_fused (tower_fm_fusable, sums): the per-layer path with first order + FM inside a gathered
    split-GEMM layer 1 -- no encoder_fm stage, and (fm_y1 = 2 on a w-ring tile) no first_order stage either."""
    L = tower_layers(c)[0] if c.fc else None
    return c.kind == "deepfm" and c.k == 16 and c.F <= ROW_OWNER_MAX_F and len(c.fc) >= 2 and B > S3_COLS_MAX_B and \
        L.Npad % 208 == 0 and not row_owner_candidate(c, 0, L)


FWD_PRED = {
    "s3_narrow2": lambda c, B, n: _has(c, B, n, "s3", "narrow2"),
    "s3_wave8": lambda c, B, n: _has(c, B, n, "s3", "wave8"),
    "s3_dense16": lambda c, B, n: _has(c, B, n, "s3", "dense16"),
    "s3_mt2_gather": lambda c, B, n: _has(c, B, n, "s3", "mt2_gather"),
    "s3_wave8_gather_any": lambda c, B, n: any(e == "s3" and t == "wave8" and tower_layers(c)[i].amode == "any"
                                               for i, e, t in fwd_tiles(c, B, n)),
    "s3_dense16_K_tail": lambda c, B, n: any(e == "s3" and t == "dense16" and tower_layers(c)[i].K % 4
                                             for i, e, t in fwd_tiles(c, B, n)),
    "s3_wave8_K_tail": lambda c, B, n: any(e == "s3" and t == "wave8" and tower_layers(c)[i].K % 4
                                           for i, e, t in fwd_tiles(c, B, n)),
    "f32_small4": lambda c, B, n: _has(c, B, n, "f32", "small4"),
    "f32_large_even_v3": lambda c, B, n: _has(c, B, n, "f32", "large_even_v3"),
    "f32_large_dense": lambda c, B, n: _has(c, B, n, "f32", "large_dense"),
    "f32_large_gather": lambda c, B, n: _has(c, B, n, "f32", "large_gather"),
    "cin_2w": lambda c, B, n: any(t == "cin_2w" for _, t in cin_tiles(c, B, n)),
    "cin_4w": lambda c, B, n: any(t == "cin_4w" for _, t in cin_tiles(c, B, n)),
    "cin_8w": lambda c, B, n: any(t == "cin_8w" for _, t in cin_tiles(c, B, n)),
    "cin_mt2": lambda c, B, n: any(t == "cin_mt2" for _, t in cin_tiles(c, B, n)),
    "cin_f32_lt_8192": lambda c, B, n: any(t == "cin_f32_lt_8192" for _, t in cin_tiles(c, B, n)),
    "cin_f32_ge_8192": lambda c, B, n: any(t == "cin_f32_ge_8192" for _, t in cin_tiles(c, B, n)),
    "cin_f32_ge_8192_odd_maps": lambda c, B, n: any(t == "cin_f32_ge_8192" and c.cin[i] % 4
                                                    for i, t in cin_tiles(c, B, n)),
    "deepfm_fm_fused_layer1": lambda c, B, n: deepfm_fm_fused_layer1(c, B),
    "deepfm_leaves_cols32": lambda c, B, n: encoder_fm_x(c) and B > S3_COLS_MAX_B and c.fc[0] != 400,
}
BF16_PRED = {
    "bf16_small4": lambda c, B, n: _has(c, B, n, "bf16", "small4", True),
    "bf16_large_even_v3": lambda c, B, n: _has(c, B, n, "bf16", "large_even_v3", True),
    "bf16_large_dense": lambda c, B, n: _has(c, B, n, "bf16", "large_dense", True),
    "bf16_large_gather": lambda c, B, n: _has(c, B, n, "bf16", "large_gather", True),
    "bf16_large_nt26": lambda c, B, n: _has(c, B, n, "bf16", "large_nt26", True),
}


# -- backward (train.hip) --
def wgrads(c):
    """[(N, K, bias, w_off, b_off)] of every dW = A^T X that reads its X (the CIN's generated operand aside): the
    tower's Linears by K block with the offsets in mats that the dW and the fused bias gradient are written at
    (linears(); b_off None where no bias rides the dW), then the DCN's cross dots (N = depth + 1 over K = F k,
    lda = depth + 1, written to a scratch buffer of its own: offset 0)."""
    blocks = [(L.Neff, K, L.bias_fusable and q == 0) for L in tower_layers(c) for q, K in enumerate(L.blocks)]
    lins = linears(c)[0]
    assert [(N, K) for N, K, _ in blocks] == [(L.N, L.K) for L in lins], c.name
    out = [(N, K, b, L.w_off, L.b_off if b else None) for (N, K, b), L in zip(blocks, lins)]
    if c.kind == "dcn":
        out.append((c.cross + 1, c.F * c.k, False, 0, None))
    return out


def wgrad_sq(B):
    return B >= WGRAD_SQ_ROWS


def wgrad_sq_slices(rows, N, K, ncu=NCU):
    """train.hip wgrad_sq_slices at wgrad_smodel = 1 (rmx_debug_wgrad_slices)."""
    tiles = ((N + 207) // 208) * ((K + 207) // 208)
    S, best = 8, -1.0
    for s8 in range(8, 513, 8):
        chunks = _up((rows + s8 - 1) // s8, 32) // 32
        rounds = (tiles * s8 + ncu - 1) // ncu
        cost = 3.8 * float(rounds * chunks) + float(s8) * N * K * 8.0 / 4.0e6
        if best < 0 or cost < best:
            best, S = cost, s8
        if chunks <= 1:
            break
    return S


def wgrad_s3_slices(rows, N, K):
    """train.hip wgrad: the slice count of the 128 x 128 tiles, and the rows of a slice."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    S = max((rows + 1023) // 1024, min((1024 + tiles - 1) // tiles, max(1, rows // 64)))
    S = _up(min(S, 512), 8)
    return S, _up((rows + S - 1) // S, 32)


def reduce_float4(N, K, bias, w_off, b_off):
    """train.hip wgrad: slice_reduce4_kernel when the dW (and the fused bias) are whole float4s and 16-byte
    aligned where they are written: g_mats + w_off, g_mats + b_off (the tests hand over a g_mats array that is
    itself aligned; the S partial planes are, S being a multiple of 8)."""
    return N * K % 4 == 0 and w_off % 4 == 0 and (not bias or (N % 4 == 0 and b_off % 4 == 0))


def head_float4(c):
    """train.hip model_train: the head's dW_out passes on float4s -- Nh % 4 == 0 and g_mats + wo_off aligned."""
    wo_off, nh = linears(c)[1]
    return nh % 4 == 0 and wo_off % 4 == 0


def head_blocks(B):
    """train.hip head_train_kernel's grid: (np, rows per block)."""
    nparts = min(1024, (B + 15) // 16)
    per = (B + nparts - 1) // nparts
    return (B + per - 1) // per, per


def head_fused(c):
    return c.kind != "lr" and c.fc[-1] <= HEAD_MAX_N


def head_two_pass(c, B):
    np_, _ = head_blocks(B)
    return head_fused(c) and np_ % 16 == 0 and np_ >= 64


def dx_s3_layers(c):
    """Layers whose dX runs on the split GEMM (dx_s3_usable, and the mask's row stride): M = B, K = the layer's
    N, Npad = NTpad, dense A.  Layer 1 only where an embedding gradient is asked for (always, in the tests)."""
    out = []
    for i, L in enumerate(tower_layers(c)):
        if L.NTpad and L.NTpad <= L.ldin and not row_owner_candidate(c, i, L):
            out.append((i, L))
    return out


def emb_fused(c):
    """train.hip: DeepFM's embedding gradient in the layer-1 dX epilogue (the FM sums need k = 16)."""
    return c.kind == "deepfm" and c.k == 16 and any(i == 0 and L.ldin == c.F * c.k for i, L in dx_s3_layers(c))


def cin_rc(c, B):
    """train.hip ensure_train: rows of one chunk of the CIN backward (a 64 M-float budget)."""
    R, hp, maxFH = B * c.k, c.F, 16
    for h in c.cin:
        maxFH, hp = max(maxFH, c.F * hp, _up(c.F * hp, 208)), h
    return min(R, max(c.k, (64 << 20) // maxFH // c.k * c.k))


def cin_rc_chunks(c, B):
    return -(-B * c.k // cin_rc(c, B)) if c.kind == "xdeepfm" else 0


BWD_PRED = {
    "wgrad_sq": lambda c, B, n: wgrad_sq(B) and bool(wgrads(c)),
    "sq_edge_n": lambda c, B, n: wgrad_sq(B) and any(N % 208 for N, K, b, _w, _b in wgrads(c)),
    "sq_edge_k": lambda c, B, n: wgrad_sq(B) and any(K % 208 for N, K, b, _w, _b in wgrads(c)),
    "sq_edge_n_one_column": lambda c, B, n: wgrad_sq(B) and any(N % 208 == 1 for N, K, b, _w, _b in wgrads(c)),
    "sq_bias_fused": lambda c, B, n: wgrad_sq(B) and any(b for N, K, b, _w, _b in wgrads(c)),
    "sq_no_bias": lambda c, B, n: wgrad_sq(B) and any(not b for N, K, b, _w, _b in wgrads(c)),
    "reduce_float4": lambda c, B, n: wgrad_sq(B) and any(reduce_float4(*w) for w in wgrads(c)),
    "reduce_float4_bias": lambda c, B, n: wgrad_sq(B) and any(reduce_float4(*w) and w[2] for w in wgrads(c)),
    "reduce_scalar": lambda c, B, n: wgrad_sq(B) and any(not reduce_float4(*w) for w in wgrads(c)),
    "reduce_scalar_NK_odd": lambda c, B, n: wgrad_sq(B) and any(N * K % 4 for N, K, b, _w, _b in wgrads(c)),
    "wgrad_128_many_slices": lambda c, B, n: not wgrad_sq(B) and any(
        wgrad_s3_slices(B, N, K)[0] >= 256 and B % wgrad_s3_slices(B, N, K)[1] for N, K, b, _w, _b in wgrads(c)),
    "wgrad_128_512_slices": lambda c, B, n: not wgrad_sq(B) and any(
        wgrad_s3_slices(B, N, K)[0] == 512 and B % wgrad_s3_slices(B, N, K)[1] for N, K, b, _w, _b in wgrads(c)),
    "emb_fused_F_26": lambda c, B, n: emb_fused(c) and c.F == 26,
    "head_two_pass_scalar": lambda c, B, n: head_two_pass(c, B) and c.fc[-1] % 4 != 0 and B % head_blocks(B)[1] != 0,
    "head_two_pass_float4": lambda c, B, n: head_two_pass(c, B) and head_float4(c),
    # Nh % 4 == 0 but W_out starts off a 16-byte boundary in mats: scalar after all
    "head_two_pass_unaligned": lambda c, B, n: head_two_pass(c, B) and c.fc[-1] % 4 == 0 and not head_float4(c),
    "reduce_scalar_unaligned": lambda c, B, n: wgrad_sq(B) and any(
        N * K % 4 == 0 and (not b or N % 4 == 0) and not reduce_float4(N, K, b, w, bo) for N, K, b, w, bo in wgrads(c)),
    "head_one_pass": lambda c, B, n: head_fused(c) and not head_two_pass(c, B),
    "tower_head_path": lambda c, B, n: c.kind != "lr" and not head_fused(c),
    "dx_s3_wave8": lambda c, B, n: any(L.Neff % 4 and s3_tile(B, L.NTpad, "dense", n) == "wave8"
                                       for _, L in dx_s3_layers(c)),
    "dx_s3_mt2": lambda c, B, n: any(L.Neff % 4 and s3_blocks2(B, L.NTpad) >= 256 for _, L in dx_s3_layers(c)),
    "cin_rc_chunks_2": lambda c, B, n: cin_rc_chunks(c, B) >= 2 and B * c.k % cin_rc(c, B) != 0,
    "cin_dz_blocks2": lambda c, B, n: c.kind == "xdeepfm" and any(
        s3_blocks2(min(B * c.k, cin_rc(c, B)), _up(c.F * hp, 208)) >= 256 and h % 4
        for hp, h in zip((c.F,) + c.cin, c.cin)),
    "cin_dz_wave8": lambda c, B, n: c.kind == "xdeepfm" and any(
        s3_tile(min(B * c.k, cin_rc(c, B)), _up(c.F * hp, 208), "dense", n) == "wave8" and h % 4
        for hp, h in zip((c.F,) + c.cin, c.cin)),
    # the training forward stores every CIN layer's maps: a split CIN layer (Npad 208) that is the last one at
    # inference or not, and the generated-operand dW over its 200 maps
    "cin_split_backward": lambda c, B, n: c.kind == "xdeepfm" and any(cin_npad(h) == 208 for h in c.cin),
    "emb_fused": lambda c, B, n: emb_fused(c),
    "cross_wgrad_sq": lambda c, B, n: wgrad_sq(B) and c.kind == "dcn",
    "pnn_two_blocks": lambda c, B, n: wgrad_sq(B) and c.kind == "pnn",
}

# the backward runs of test_batch_sweep.py: the f64 oracle takes the whole batch, so a chosen list (oracle seconds
# per run in DESIGN.md §4).  BWD_KNOB_ROWS: the rows of the knob cross-check; BWD_LEFTOVER_ROWS: the K-tail rows
BWD_RUNS = (
    ("dnn_f5k4_37x400", B33K), ("dnn_f5k4_37x400", 16400), ("dnn_f5k4_413x401", B33K),
    ("deepfm_f7k10_33x20", B33K), ("deepfm_f13k16_209x37", B33K), ("deepfm_f13k16_401x37", B33K),
    ("dnn_f9k16_24x8x200x7x16", B33K), ("dnn_f9k16_24x8x200x7x16", 65573), ("dnn_f3k32_520", B33K),
    ("dcn_f7k10_33x20_d3", B33K), ("pnn_f7k10_33x20", B33K),
    ("xdeepfm_f5k16_100x37_cin10x7", 2048), ("xdeepfm_f5k16_100x37_cin10x7", 4099),
    ("xdeepfm_f17k16_500x7_cin256x3", 1024), ("xdeepfm_f5k16_33_cin200x7", 4099),
    # 32,500: the last batches before the 208 x 208 tile give the 128 x 128 dW its 512 slices (rows / 64 >= 505);
    # F = 26 (F 16 = 416) with the embedding gradient in the layer-1 dX epilogue: a small batch, the path takes none
    ("dnn_f5k4_37x400", 32500), ("deepfm_f26k16_413x20", 2049),
)
# (slice_reduce4 changes the kernels launched on the second and third: the dW with its bias, the head's two passes)
BWD_KNOB_ROWS = ("dnn_f5k4_37x400", "dnn_f9k16_24x8x200x7x16", "pnn_f7k10_33x20")
# with wgrad_s3 0 the CIN's dW is no longer one launch over all B k rows with its operand generated: each chunk of
# the CIN backward materialises z and adds its dW to the chunks before (accum, r0 > 0) -- two chunks here
CIN_ACCUM_RUN = ("xdeepfm_f17k16_500x7_cin256x3", 1024)
BWD_LEFTOVER_ROWS = ("dnn_f9k16_24x8x200x7x16", "dnn_f5k4_413x401")

# (row, batch, the predicates that run claims for): forward claims need the batch on the row's ladder, bf16 claims
# on BF16_LADDER, backward claims the pair in BWD_RUNS
CLAIMS = (
    ("dnn_f5k4_413x401", 2049, "s3_narrow2"),
    ("dnn_f5k4_413x401", 16400, "s3_wave8 s3_wave8_gather_any s3_wave8_K_tail"),
    ("dnn_f5k4_413x401", B33K, "s3_dense16 s3_dense16_K_tail s3_wave8_gather_any"),
    ("dnn_f5k4_37x400", B33K, "s3_dense16_K_tail f32_small4"),
    ("deepfm_f13k16_401x37", 2049, "deepfm_fm_fused_layer1 deepfm_leaves_cols32 s3_narrow2"),
    ("deepfm_f13k16_401x37", 16400, "deepfm_fm_fused_layer1 s3_wave8"),
    ("deepfm_f13k16_401x37", B33K, "deepfm_fm_fused_layer1 s3_mt2_gather"),
    ("deepfm_f26k16_413x20", 65573, "deepfm_fm_fused_layer1 s3_mt2_gather f32_large_dense"),
    ("deepfm_f39k16_832x200", 16400, "deepfm_fm_fused_layer1 s3_mt2_gather"),
    ("deepfm_f13k16_209x37", 2049, "deepfm_leaves_cols32 f32_small4"),
    ("deepfm_f17k8_500x7", 65573, "f32_large_even_v3 f32_large_dense"),
    ("deepfm_f5k4_100x37", 65573, "f32_large_gather f32_large_dense"),
    ("xdeepfm_f5k16_33_cin200x7", 509, "cin_2w cin_f32_lt_8192"),
    ("xdeepfm_f5k16_33_cin200x7", 1024, "cin_4w cin_f32_ge_8192"),
    ("xdeepfm_f5k16_33_cin200x7", 2048, "cin_8w"),
    ("xdeepfm_f5k16_33_cin200x7", 4099, "cin_mt2"),
    ("xdeepfm_f5k16_33_cin200x7", 16400, "cin_mt2 cin_f32_ge_8192_odd_maps"),
    ("xdeepfm_f5k16_100x37_cin10x7", 16400, "cin_f32_ge_8192_odd_maps"),
    ("dnn_f5k4_413x401", 16400, "bf16_small4"),
    ("dnn_f5k4_413x401", 65573, "bf16_large_nt26"),
    ("deepfm_f17k8_500x7", 65573, "bf16_large_even_v3 bf16_large_dense"),
    ("dnn_f17k8_500x7", 65573, "bf16_large_even_v3"),
    ("dcn_f17k16_64x32_d3", 65573, "bf16_large_gather bf16_large_dense"),
    # (layer 2's W starts at 20 37 + 37 = 777 in mats and W_out at 15,977: whole float4s, but off a 16-byte boundary)
    ("dnn_f5k4_37x400", B33K, "wgrad_sq sq_edge_n sq_edge_k sq_bias_fused reduce_scalar reduce_scalar_unaligned "
                              "head_two_pass_unaligned"),
    ("dnn_f5k4_37x400", 16400, "wgrad_128_many_slices head_one_pass"),
    ("dnn_f5k4_413x401", B33K, "wgrad_sq sq_edge_n sq_edge_k reduce_scalar dx_s3_mt2 head_two_pass_scalar"),
    ("deepfm_f7k10_33x20", B33K, "reduce_scalar_NK_odd sq_bias_fused"),
    ("deepfm_f13k16_209x37", B33K, "emb_fused head_two_pass_scalar sq_edge_n_one_column reduce_scalar"),
    ("deepfm_f13k16_401x37", B33K, "emb_fused sq_edge_n reduce_scalar"),
    ("dnn_f9k16_24x8x200x7x16", B33K, "dx_s3_wave8 reduce_float4 reduce_float4_bias"),  # offsets 0 / 3,456 / 3,480 ...
    ("dnn_f9k16_24x8x200x7x16", 65573, "dx_s3_mt2 head_one_pass"),
    ("dnn_f3k32_520", B33K, "tower_head_path wgrad_sq"),
    ("dcn_f7k10_33x20_d3", B33K, "cross_wgrad_sq sq_no_bias"),
    ("pnn_f7k10_33x20", B33K, "pnn_two_blocks sq_no_bias reduce_float4_bias head_two_pass_float4"),
    ("xdeepfm_f5k16_100x37_cin10x7", 2048, "cin_dz_wave8"),
    ("xdeepfm_f5k16_100x37_cin10x7", 4099, "cin_dz_blocks2"),
    ("xdeepfm_f17k16_500x7_cin256x3", 1024, "cin_rc_chunks_2"),
    ("xdeepfm_f5k16_33_cin200x7", 4099, "cin_dz_blocks2 cin_split_backward"),
    ("dnn_f5k4_37x400", 32500, "wgrad_128_512_slices"),
    ("deepfm_f26k16_413x20", 2049, "emb_fused_F_26"),
)


def claims_of(names):
    """[(row, batch, predicate)] of CLAIMS for the predicates in `names`."""
    return [(r, B, p) for r, B, ps in CLAIMS for p in ps.split() if p in names]


# ---- the mats layout (models.hip mats_sizes) -------------------------------------------------------------
Linear = collections.namedtuple("Linear", "what w_off K N b_off")  # W = mats[w_off : w_off + N K] as [N][K]


def linears(c):
    """Every hidden Linear of the tower (PNN's layer 1 as its two blocks, the x block and the product block,
    which share one scalar bias: b_off None) and the slice (offset, length) of the output Linear's weights that
    multiplies the last hidden layer."""
    F, k, D = c.F, c.k, c.F * c.k
    if c.kind == "lr":
        return [], (0, 0)
    lin, off, prev, fc = [], 0, D, c.fc
    if c.kind == "dcn":
        off = c.cross * D + c.cross
    if c.kind == "pnn":
        P, D1 = F * (F - 1) // 2, fc[0]
        lin.append(Linear("layer1_x", 0, D, D1, None))
        lin.append(Linear("layer1_product", D * D1, P, D1, None))
        off, prev, fc = (D + P) * D1 + 1, D1, fc[1:]
    for i, d in enumerate(fc):
        lin.append(Linear("layer%d" % (i + 1 + (c.kind == "pnn")), off, prev, d, off + prev * d))
        off, prev = off + prev * d + d, d
    if c.kind == "xdeepfm":
        hp = F
        for h in c.cin:
            off, hp = off + F * hp * h + h, h
        off += sum(c.cin)
    if c.kind == "dcn":
        off += D
    return lin, (off, prev)


# ---- models, parameters, inputs and references, each made once and handed out read-only ------------------
def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def orc_model(name):
    c = BY_NAME[name]
    return oc.make_model(ORC[c.kind], c.F, c.k, fc=c.fc, cin=c.cin, cross_depth=c.cross)


@functools.lru_cache(None)
def host_mats(name, bf16=False):
    """initMats, the output weights over the last hidden layer times the row's power of two `scale`; a bf16 model
    is given mats already rounded to bf16, as in test_bf16.py."""
    c = BY_NAME[name]
    if c.kind == "lr":
        return _ro(np.zeros(0, np.float32))
    mats = oc.init_mats(orc_model(name), c.mseed)
    assert len(mats) == oc.mats_len(orc_model(name))
    off, n = linears(c)[1]
    mats[off:off + n] *= np.float32(c.scale)
    return _ro(oc.round_bf16(mats) if bf16 else mats)


def rmx_model(name, bf16=False, V_=V):
    """A new rmx model of the row with its parameters set (fp32, or bf16 storage on rounded mats)."""
    import rmx
    c = BY_NAME[name]
    fc, cin = list(c.fc), list(c.cin)
    m = {"lr": lambda: rmx.LR(V_, c.F), "deepfm": lambda: rmx.DeepFM(V_, c.F, c.k, fc),
         "dnn": lambda: rmx.DNN(V_, c.F, c.k, fc), "dcn": lambda: rmx.DCN(V_, c.F, c.k, c.cross, fc),
         "pnn": lambda: rmx.PNN(V_, c.F, c.k, fc), "xdeepfm": lambda: rmx.XDeepFM(V_, c.F, c.k, fc, cin)}[c.kind]()
    if bf16:
        m.setPrecision(rmx.DTYPE_BF16)
    if c.kind != "lr":
        m.setMats(host_mats(name, bf16))
    m.setBias(BIAS)
    return m


@functools.lru_cache(None)
def host_table(k, bf16=False):
    wt, et = oc.gen_table(SEED_TAB, V, k)
    if bf16:
        wt, et = oc.round_bf16(wt), oc.round_bf16(et)
    return _ro(wt), _ro(et)


_tables = {}


def dev_table(ctx, k, bf16=False):
    """The synthetic table of k columns on the device (fill_synthetic: gen_table's bits, rounded for bf16)."""
    import rmx
    if (k, bf16) not in _tables:
        t = rmx.EmbeddingTable(ctx, V, k, rmx.DTYPE_BF16 if bf16 else rmx.DTYPE_F32)
        t.fill_synthetic(SEED_TAB)
        _tables[k, bf16] = t
    return _tables[k, bf16]


@functools.lru_cache(None)
def host_ids(F, B, row0=0):
    return _ro(oc.gen_ids(SEED_IDS, row0, B, F, V).astype(np.int32))


def index_of(B, F):
    return np.repeat(np.arange(B, dtype=np.int64), F)


def rows_of(c, ids, bf16=False):
    """(w, e): the table gather of ids -- what a host-array caller passes as weights / embeddings."""
    wt, et = host_table(c.k, bf16)
    return oc.gather(wt, et, 1, np.asarray(ids, np.int64).reshape(-1))


def oracle_on(c, ids, precision, bf16=False, mats=None):
    """The oracle's probabilities of the rows `ids` ([B][F]): precision 0 fp32, 1 fp64, 2 the bf16 emulation;
    bf16: on the bf16-rounded table and mats."""
    ids = np.asarray(ids).reshape(-1, c.F)
    B = ids.shape[0]
    w, e = rows_of(c, ids, bf16)
    lr = c.kind == "lr"
    if mats is None:
        mats = host_mats(c.name, bf16)
    return oc.forward(orc_model(c.name), B, index_of(B, c.F), np.array([BIAS], np.float32), w, None if lr else e,
                      None if lr else mats, precision)


@functools.lru_cache(None)
def oracle_forward(name, B, precision, bf16=False, row0=0):
    c = BY_NAME[name]
    return _ro(oracle_on(c, host_ids(c.F, B, row0), precision, bf16))


# ---- backward --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def host_targets(B):
    return _ro((np.random.default_rng(5).random(B) > 0.7).astype(np.float32))


@functools.lru_cache(None)
def tie_free_rows(name, ncand):
    """Indices, among the ncand candidate rows gen_ids makes from the row's id seed (row0), of the rows whose
    ReLU inputs all stay clear of zero (grad_check._tie_free)."""
    from grad_check import _tie_free
    c = BY_NAME[name]
    if c.kind == "lr":
        return _ro(np.arange(ncand))
    cand = host_ids(c.F, ncand, c.row0).reshape(ncand, c.F).astype(np.int64)
    _, et = host_table(c.k)
    step = 64 if c.kind == "xdeepfm" else 4096  # the CIN's z rows are [rows k][F Hp] f64
    keep = [r0 + _tie_free(c.kind, et[cand[r0:r0 + step]].astype(np.float64), host_mats(name), c.fc, cross=c.cross,
                           cin=c.cin) for r0 in range(0, ncand, step)]
    return _ro(np.concatenate(keep))


@functools.lru_cache(None)
def tie_free_ids(name, B):
    """B tie-free rows of ids picked from 4 B candidates."""
    c = BY_NAME[name]
    keep = tie_free_rows(name, 4 * B)
    assert len(keep) >= B, (name, B, len(keep))
    return _ro(np.ascontiguousarray(host_ids(c.F, 4 * B, c.row0).reshape(4 * B, c.F)[keep[:B]]))


def _oracle_backward_on(c, ids, targets):
    n = len(targets)
    w, e = rows_of(c, ids)
    return oc.backward(orc_model(c.name), n, index_of(n, c.F), np.array([BIAS], np.float32),
                       w if c.kind != "dnn" else None, e if c.kind != "lr" else None,
                       host_mats(c.name) if c.kind != "lr" else None, targets)


@functools.lru_cache(None)
def oracle_backward(name, B):
    return _oracle_backward_on(BY_NAME[name], tie_free_ids(name, B), host_targets(B))


def oracle_mats_share(name, B, n):
    """The share of the last n rows of the (name, B) backward batch in its mats gradient: the oracle on those rows
    alone (a mean over n) times n / B.  A kernel that drops them from its batch sums is off by exactly this."""
    g = _oracle_backward_on(BY_NAME[name], tie_free_ids(name, B)[B - n:], host_targets(B)[B - n:])
    return g["mats"].astype(np.float64) * (n / B)


def close_bars(move, ref, rel=2e-5, rtol=1e-3, floor=1e-3):
    """`move` against grad_check._close's two bars around ref: (max |move| / max |ref|) / rel and the largest
    |move| / element-wise bound -- either above 1 fails _close."""
    ref, move = np.abs(np.asarray(ref, np.float64)), np.abs(np.asarray(move, np.float64))
    mx = max(float(ref.max()), 1e-6)
    return float(move.max()) / mx / rel, float((move / (rtol * np.maximum(ref, floor * mx))).max())
