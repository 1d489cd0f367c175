"""GPU: the exact probe networks of tests/split_probes.py through every fp32 path of a 400^3 DeepFM tower.

Each probe makes ONE part product of the 3-way bf16 split (or the unrounded bias, or the sign) the whole tower
output: kept, the logit is 1 + b_out + beta; dropped, it is b_out + beta, more than 0.1 away in p
(test_split_probes_cpu.py proves both against the oracle alone).  Every kernel that splits activations in
registers and walks the weight planes must therefore return sigmoid(expected_logit) to within the head's expf
(4 ulp of p), at every K position and every column of every layer, for rows in every place of a 16-row wave and
of a 128-row block:

    cols       the column-split small-batch path (k_gemm_s3.hip cols32 tiles), default knobs, B <= 2,048
    small      the whole-tower kernel (k_small_s3.hip), s3_small 2
    fused      the fused tower (k_fused_s3.hip), s3_fused 2
    head_tail  layer 1 + layers 2, 3 row-owner kernels (k_head_s3.hip, k_tail_s3.hip)
    generic    the per-layer split GEMM (k_gemm_s3.hip), the four knobs above 0
    f32_mfma   the fp32 MFMA engine (f32_split 0): exact as well

The path is forced by knobs and confirmed by the timed stage list.  One round per layer also runs on the line
table (table_lines 1), with half row blocks on and off, on the other tiles of the per-layer and column-split
GEMMs (s3_narrow, s3_tower, s3_cols_wm), and through the host-array entry forward(...) (implicit ids)."""
import numpy as np
import pytest

import rmx
import split_probes as sp

pytestmark = pytest.mark.gpu

ULPS = 4

# path: (knobs, stages that must appear, stages that must not)
PATHS = {
    "cols": ({}, ("encoder_fm_x", "tower_layer1", "tower_layer2", "tower_layer3"), ("tower_small", "tower_fused")),
    "small": ({"s3_small": 2}, ("tower_small",), ("encoder_fm_x", "tower_layer1", "tower_fused")),
    "fused": ({"s3_fused": 2, "s3_small": 0}, ("tower_fused",), ("encoder_fm_x", "tower_layer1", "tower_small")),
    "head_tail": ({"s3_fused": 0, "s3_head": 2, "s3_tail": 2, "s3_small": 0}, ("tower_layer1", "tower_tail"),
                  ("encoder_fm_x", "tower_small", "tower_fused", "tower_layer2")),
    "generic": ({"s3_fused": 0, "s3_head": 0, "s3_tail": 0, "s3_small": 0},
                ("tower_layer1", "tower_layer2", "tower_layer3"),
                ("encoder_fm_x", "tower_small", "tower_fused", "tower_tail")),
    "f32_mfma": ({"f32_split": 0}, ("tower_layer1", "tower_layer2", "tower_layer3"),
                 ("encoder_fm_x", "tower_small", "tower_fused", "tower_tail")),
}
KNOBS = ("s3_small", "s3_fused", "s3_head", "s3_tail", "f32_split", "table_lines", "half_blocks", "s3_tower",
         "s3_narrow", "s3_cols_wm")


@pytest.fixture(scope="module")
def ctx():
    return rmx.default_context()


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    for k in KNOBS:
        rmx.set_tuning(k, None)


def _set_path(path, **extra):
    for k in KNOBS:
        if k != "table_lines":  # (read when a table is uploaded: set by the caller around the upload)
            rmx.set_tuning(k, None)
    for k, v in dict(PATHS[path][0], **extra).items():
        rmx.set_tuning(k, v)


def _check(rd, B, got, what):
    want = sp.sigmoid32(rd.expected_logit[:B])
    tol = ULPS * np.spacing(want).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s, B = %d\n%s" % (what, B, sp.describe(rd, bad, got, want))


class _Round:
    """A probe round on the device: the model with its mats, the uploaded table, the ids."""

    def __init__(self, ctx, probe, layer, rnd, lines=0, change=None):
        self.ctx = ctx
        self.Bmax = max(sp.batches(layer))
        rd = sp.build(probe, layer, rnd, self.Bmax)  # (a smaller batch is a prefix of its rows)
        self.rd = rd = change(rd) if change else rd
        self.m = rmx.DeepFM(rd.V, sp.F, sp.K, list(sp.FC))
        self.m.setMats(rd.mats)
        self.m.setBias(rd.bias)
        rmx.set_tuning("table_lines", lines)
        self.table = rmx.EmbeddingTable(ctx, rd.V, sp.K)
        self.table.upload(rd.w_table, rd.emb_table)  # (builds the line copy when the knob asks for one)
        self.ids = rmx.DeviceArray.from_numpy(ctx, rd.ids.ravel())
        self.out = rmx.DeviceArray(ctx, self.Bmax, np.float32)

    def run(self, path, B, **extra):
        _set_path(path, **extra)
        m = self.m
        m.set_timing(True)
        m.forward_ids(self.table, B, self.ids, self.out)
        self.ctx.sync()
        stages, _ = m.get_timing()
        m.set_timing(False)
        need, never = PATHS[path][1:]
        assert all(s in stages for s in need) and not any(s in stages for s in never), (path, list(stages))
        _check(self.rd, B, self.out.numpy()[:B].copy(), "path %s %s" % (path, extra or ""))


@pytest.mark.parametrize("layer", sp.LAYERS)
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_probe_exact_on_every_fp32_path(ctx, probe, layer):
    for rnd in range(sp.ROUNDS):
        r = _Round(ctx, probe, layer, rnd)
        for B in sp.batches(layer):
            for path in PATHS:
                r.run(path, B)


@pytest.mark.parametrize("layer", sp.LAYERS)
def test_probes_on_line_table_half_blocks_tiles_and_host_arrays(ctx, layer):
    rnd = layer % sp.ROUNDS
    for probe in sp.PROBES:
        B = sp.batches(layer)[1]
        # the [V][32] line copy of the table (row and weight strides 32)
        r = _Round(ctx, probe, layer, rnd, lines=1)
        for path in PATHS:
            r.run(path, B)
        # half row blocks of the row-owner kernels (k_rowown.hpp) on and off
        r = _Round(ctx, probe, layer, rnd)
        for hb in (0, 1):
            for path in ("fused", "head_tail"):
                r.run(path, B, half_blocks=hb)
        # the other tiles of the per-layer split GEMM (k_gemm_s3.hip launch_tower_s3: the 8-wave tile instead of
        # the 2-wave one small batches take, the register-staged and the two single-buffered variants) and the
        # other block heights of the column-split tiles
        for extra in ({"s3_narrow": 0}, {"s3_tower": 2}, {"s3_tower": 3}, {"s3_tower": 4}):
            r.run("generic", B, **extra)
        for wm in (2, 8):
            r.run("cols", B, s3_cols_wm=wm)
        # the host-array entry (RecModel.forward): staged rows with implicit ids, column-split path by default,
        # the whole-tower kernel when forced
        rd = r.rd
        index, w, e = sp.gathered(rd)
        m = rmx.DeepFM(rd.V, sp.F, sp.K, list(sp.FC))
        for path in ("cols", "small"):
            _set_path(path)
            m.set_timing(True)
            got = m.forward(B, rmx.CooLongFloatMatrix(index, rd.ids.ravel()), rd.bias, w, e, sp.K, rd.mats,
                            m.getMatsSize())
            stages, _ = m.get_timing()
            m.set_timing(False)
            assert ("tower_small" if path == "small" else "encoder_fm_x") in stages, (path, list(stages))
            _check(rd, B, np.asarray(got, np.float32), "host arrays, path %s" % path)


def _hi_mid(a):
    hi, mid, _ = sp.split3(a)
    return (hi + mid).astype(np.float32)


@pytest.mark.parametrize("layer", sp.LAYERS)
@pytest.mark.parametrize("probe,cut", [("act_hi_w_lo", "mats"), ("act_lo_w_hi", "table"), ("bias", "table")])
def test_probe_loses_its_one_when_the_operand_loses_lo(ctx, probe, cut, layer):
    """The converse, on the device: with the lo part cut from the probed operand on the host (the weights, or the
    table rows, rounded to hi + mid) every path must return sigmoid(b_out + beta) -- the 1 in the logit reaches
    the output through the lo part and the kernels' lo products, not by another way."""
    def change(rd):
        lost = rd.expected_logit - sp.PROBES[probe].kept
        if cut == "mats":
            return rd._replace(mats=_hi_mid(rd.mats), expected_logit=lost)
        return rd._replace(emb_table=_hi_mid(rd.emb_table.ravel()).reshape(rd.emb_table.shape), expected_logit=lost)

    r = _Round(ctx, probe, layer, 0, change=change)
    for path in PATHS:
        r.run(path, sp.batches(layer)[0])
