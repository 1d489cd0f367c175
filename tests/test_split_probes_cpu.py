"""CPU proof that the exact probe networks of tests/split_probes.py test what they say (no GPU).

1. Every probe round is exact: the fp64 oracle and the fp32 oracle (sequential fp32 sums) both return
   sigmoid(expected_logit) bit for bit, and so does the numpy restatement with the 6-product split.
2. Every probe is sensitive to its product: with ONE of the six products removed from the probed layer's
   split Linear (split_probes.split_linear; in the other layers hi x hi carries the routing), exactly the
   probes that name it in Probe.flips lose the tower's 1 in the logit (p = sigmoid(b_out + beta) instead of
   sigmoid(1 + b_out + beta): more than 0.1 away); every other probe keeps its bits.
3. The rounds cover every K position and every real column of every layer, and no two samples of a round share
   a weight entry (asserted inside build()).
"""
import numpy as np
import pytest

import oracle_ctypes as oc
import split_probes as sp

OM = oc.make_model(oc.DEEPFM, sp.F, sp.K, fc=sp.FC)


def _distinct(probe, layer, rnd):
    return sp.build(probe, layer, rnd, sp.n_distinct(layer))


@pytest.mark.parametrize("layer", sp.LAYERS)
@pytest.mark.parametrize("probe", list(sp.PROBES))
def test_probe_rounds_are_exact_in_both_oracles(probe, layer):
    for rnd in range(sp.ROUNDS):
        B = sp.batches(layer)[rnd % 2]  # (the repeats of the larger batches share ids with these rows)
        rd = sp.build(probe, layer, rnd, B)
        assert rd.mats.size == oc.mats_len(OM)
        index, w, e = sp.gathered(rd)
        want = sp.sigmoid32(rd.expected_logit)
        for precision in (1, 0):
            got = oc.forward(OM, B, index, rd.bias, w, e, rd.mats, precision)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "oracle precision %d\n%s" % (precision, sp.describe(rd, bad, got, want))
        # kept / dropped / a head without b_out or beta are all different fp32 values of p
        pr = sp.PROBES[probe]
        alts = {float(sp.sigmoid32(v)) for v in (pr.kept + sp.B_OUT + sp.BETA, 1 - pr.kept + sp.B_OUT + sp.BETA,
                                                 pr.kept + sp.B_OUT, pr.kept + sp.BETA, pr.kept)}
        assert len(alts) == 5


@pytest.mark.parametrize("layer", sp.LAYERS)
def test_each_probe_flips_without_its_product_and_only_then(layer):
    for probe, pr in sp.PROBES.items():
        rd = _distinct(probe, layer, 1)
        B = rd.ids.shape[0]
        index, w, e = sp.gathered(rd)
        args = ("deepfm", B, sp.F, sp.K, index, rd.bias, w, e, rd.mats)
        kept = sp.sigmoid32(rd.expected_logit)
        dropped = sp.sigmoid32(rd.expected_logit - pr.kept)
        p = sp.forward_split(sp.PRODUCTS6, *args, fc=sp.FC).astype(np.float32)
        assert np.array_equal(p, kept), probe
        for gone in sp.PRODUCTS6:
            keep = tuple(q for q in sp.PRODUCTS6 if q != gone)
            p = sp.forward_split(keep, *args, only=layer, fc=sp.FC).astype(np.float32)
            if gone in pr.flips:
                # (mid_mid without hm or mh keeps an uncancelled 2^-10: another wrong p, not the dropped one)
                assert np.array_equal(p, dropped) or (probe == "mid_mid" and gone != "mm"), (probe, gone)
                assert np.abs(p.astype(np.float64) - kept).min() > 0.1, (probe, gone)
            else:
                assert np.array_equal(p, kept), (probe, gone)
    # four products are the only flip of some probe; {act_mid_w_hi, act_hi_w_mid, mid_mid} pin mid x mid down
    # together; hi x hi carries every routing layer (without it anywhere, no probe's 1 reaches the logit)
    alone = {pr.flips[0] for pr in sp.PROBES.values() if len(pr.flips) == 1}
    assert alone == {"hm", "mh", "hl", "lh"}
    assert set(sp.PROBES["mid_mid"].flips) - alone == {"mm"}
    rd = _distinct("act_lo_w_hi", layer, 0)
    index, w, e = sp.gathered(rd)
    p = sp.forward_split(tuple(q for q in sp.PRODUCTS6 if q != "hh"), "deepfm", rd.ids.shape[0], sp.F, sp.K, index,
                         rd.bias, w, e, rd.mats, fc=sp.FC)
    assert np.array_equal(p.astype(np.float32), sp.sigmoid32(rd.expected_logit - 1))


def test_omitted_products_are_zero_in_every_probe():
    """mid x lo, lo x mid and lo x lo vanish for both terms of every probe (and for the routing weights, which
    are powers of two): the 6-product split loses nothing, so the probes must be exact on it."""
    for name, pr in sp.PROBES.items():
        for x, wgt in ((pr.xa, pr.wa), (pr.xb, pr.wb)):
            xh, xm, xl = sp.split3(np.array([x], np.float32))
            wh, wm, wl = sp.split3(np.array([wgt], np.float32))
            assert float(xh[0]) + float(xm[0]) + float(xl[0]) == x and float(wh[0]) + float(wm[0]) + float(wl[0]) == wgt
            assert xm[0] * wl[0] == 0 and xl[0] * wm[0] == 0 and xl[0] * wl[0] == 0, name
            if name != "mid_mid":
                assert (xm[0] == 0 and xl[0] == 0) or (wm[0] == 0 and wl[0] == 0), name
            # truncation (the other way to cut an fp32 to bf16) splits these operands the same way
            for v, parts in ((x, (xh, xm, xl)), (wgt, (wh, wm, wl))):
                r = np.array([v], np.float32)
                for part in parts:
                    t = (r.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
                    assert t[0] == part[0], (name, v)
                    r = (r - t).astype(np.float32)


@pytest.mark.parametrize("layer", sp.LAYERS)
def test_rounds_cover_every_k_position_and_column(layer):
    kdim = sp.D if layer == 1 else 400
    for probe in sp.PROBES:
        ks, cols = set(), set()
        for rnd in range(sp.ROUNDS):
            rd = _distinct(probe, layer, rnd)
            ks |= set(rd.meta["kpos"].ravel().tolist())
            cols |= set(rd.meta["col"].tolist())
            # two nonzero inputs per sample, in different fields at different k indices; row 0 elsewhere
            nz = rd.ids != 0
            assert np.all(nz.sum(1) == 2)
            assert np.all(rd.emb_table[0] == 0) and np.all(rd.w_table == 0)
            assert np.all((rd.emb_table[1:] != 0).sum(1) <= 1)
            pos = rd.meta["pos"]
            assert np.all(pos[:, 0] // sp.K != pos[:, 1] // sp.K) and np.all(pos[:, 0] % sp.K != pos[:, 1] % sp.K)
        assert ks == set(range(kdim)), (probe, layer)
        assert cols == set(range(400)), (probe, layer)
    # the larger batches put every distinct sample into other rows of a 16-row wave and a 128-row block
    n = sp.n_distinct(layer)
    rd = sp.build("act_lo_w_hi", layer, 0, sp.batches(layer)[1])
    s = rd.meta["sample"]
    for i in (0, 1, n - 1):
        rows = np.flatnonzero(s == i)
        assert rows.size >= 2 and np.unique(rows % 16).size > 1 and np.unique(rows % 128).size > 1
