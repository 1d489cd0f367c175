"""Exact probe networks and a split-GEMM emulation for the fp32 towers -- TEST INFRASTRUCTURE ONLY.

The fp32 layers run on the bf16 matrix cores through the 3-way split x = hi + mid + lo (csrc/k_gemm_s3.hip):
six of the nine part products are kept.  Against random weights the sigmoid output hardly sees a missing
product (README "parity"); the networks built here make ONE kept product the whole answer.

A probe network is a DeepFM with F = 39, k = 16, fc = (400, 400, 400) (HigherOrderEncoder.scala:34-59,
DeepFM.scala:54-80).  Table row 0 is all zero, every first-order weight is 0.  Sample i points every field at
row 0 except two fields, each at a private row with a single nonzero element, at different k indices: the
first order and the FM are exactly 0 and the tower input has two nonzeros xa, xb.  One column c of the probed
layer computes xa wa + xb wb (+ b); the layers before it select (weight 1), the layers after it multiply by
2^10 and the output weight brings the column's value 2^-e to 1, so

    logit = 1 + b_out + beta   if the probed product is kept (and the bias added unrounded),
    logit =     b_out + beta   if it is dropped.

Every operand is a sum of at most three powers of two, every partial sum in any order is exact in fp32, and
the three products the design omits (mid lo, lo mid, lo lo) are exactly zero in every probe, so the fp64
oracle, the fp32 oracle, the f32 MFMA engine and the 6-product split must all give the same bits.

split_linear(keep) restates a Linear as the sum of the kept part products (on ref_numpy._linear, in fp64):
forward_split runs any model of ref_numpy with it, which is how the CPU tests prove what each probe is
sensitive to and how test_logit_parity gets the error of a 2-term split (the bar's yardstick).
"""
import contextlib
from typing import NamedTuple

import numpy as np

import ref_numpy
from test_split_math import split3

F, K = 39, 16
FC = (400, 400, 400)
D = F * K
N_MATS = D * 400 + 400 + 2 * (400 * 400 + 400) + 400 + 1

# part products, activation part first: "lh" = activation lo x weight hi
PRODUCTS6 = ("hh", "hm", "mh", "hl", "lh", "mm")
PRODUCTS_2TERM = ("hh", "hm", "mh", "mm")  # both operands cut to hi + mid: every product with a lo part gone

B_OUT = 0.25   # output Linear's bias
BETA = 0.125   # the model's bias: kept / dropped / a head without b_out or beta all differ in p

_A, _B9, _C = 2.0 ** -10, 2.0 ** -9, 2.0 ** -20


class Probe(NamedTuple):
    xa: float
    wa: float
    xb: float
    wb: float
    b: float      # bias of the probed column
    e: int        # the column's pre-ReLU value is +-2^-e
    kept: float   # tower contribution to the logit with every product kept
    flips: tuple  # removing any ONE of these products changes p; removing any other leaves it


# Each operand splits the same way under truncation and round-to-nearest-even (1 + 2^-10 + 2^-20: hi 1,
# mid 2^-10, lo 2^-20).  No probe has mid or lo on both operands except mid_mid, whose cross terms cannot be
# cancelled class by class with two terms (hh, hm, mh fixed => mm of the second term = -2^-20), so it also
# flips without hm or mh; act_mid_w_hi and act_hi_w_mid isolate those two, which leaves mm.
PROBES = {
    "act_lo_w_hi": Probe(1 + _A + _C, 1.0, 1 + _A, -1.0, 0.0, 20, 1.0, ("lh",)),
    "act_hi_w_lo": Probe(1.0, 1 + _A + _C, 1.0, -(1 + _A), 0.0, 20, 1.0, ("hl",)),
    "act_mid_w_hi": Probe(1 + _A, 1.0, 1.0, -1.0, 0.0, 10, 1.0, ("mh",)),
    "act_hi_w_mid": Probe(1.0, 1 + _A, 1.0, -1.0, 0.0, 10, 1.0, ("hm",)),
    "mid_mid": Probe(1 + _A, 1 + _A, 1 + _B9, -1.0, 0.0, 20, 1.0, ("hm", "mh", "mm")),
    # the second term's weight is 0: xa wa + b with b = -(1 + 2^-10) added unrounded (b is no product: it
    # cancels xa's hi and mid against wa, so those two products flip this probe as well)
    "bias": Probe(1 + _A + _C, 1.0, 1.0, 0.0, -(1 + _A), 20, 1.0, ("hh", "mh", "lh")),
    # act_lo_w_hi negated: -2^-20, ReLU returns exactly 0 (kept or dropped: p = sigmoid(b_out + beta))
    "sign": Probe(1 + _A + _C, -1.0, 1 + _A, 1.0, 0.0, 20, 0.0, ()),
}

LAYERS = (1, 2, 3)
ROUNDS = 2  # per (probe, layer): two rounds cover every column, and swap the two operands' K positions


def n_distinct(layer):
    """Distinct samples of a round: two K positions each (624 in layer 1, 400 in layers 2 and 3)."""
    return D // 2 if layer == 1 else 200


def batches(layer):
    """Ragged last wave (16 rows) and ragged 128-row block; every distinct sample at least twice."""
    return (624, 1248) if layer == 1 else (400, 1000)


class ProbeRound(NamedTuple):
    V: int
    w_table: np.ndarray    # [V] zeros
    emb_table: np.ndarray  # [V, K]
    ids: np.ndarray        # [B, F] int32
    mats: np.ndarray
    bias: np.ndarray       # [1]
    expected_logit: np.ndarray  # [B] float64
    meta: dict             # probe, layer, round, and per row: sample, pos (input positions), kpos, col


def sigmoid32(logit):
    """sigmoid in fp64, rounded once to fp32: what both oracles give for these logits."""
    return (1.0 / (1.0 + np.exp(-np.asarray(logit, np.float64)))).astype(np.float32)


def _input_positions(n):
    """Input positions (f k + j) of the two operands of samples 0 .. n-1: different fields, different j."""
    i = np.arange(n)
    pa, pb = i, D // 2 + (i + 20) % (D // 2)
    assert np.all(pa // K != pb // K) and np.all(pa % K != pb % K)
    assert np.unique(np.concatenate([pa, pb])).size == 2 * n
    return pa, pb


def _offsets():
    offs, o, dim = [], 0, D
    for d in FC:
        offs.append((o, o + dim * d, dim))  # W [d][dim], b [d]
        o += dim * d + d
        dim = d
    return offs, o  # o: w_out [400], then b_out


def build(probe, layer, rnd, B):
    """One round: probe `probe` in tower layer `layer` (1-based), round `rnd`, B rows."""
    pr = PROBES[probe]
    n = n_distinct(layer)
    swap = rnd % 2 == 1
    pa, pb = _input_positions(n)
    i = np.arange(n)
    if layer == 1:
        if swap:
            pa, pb = pb, pa
        ka, kb = pa, pb
    else:
        ka, kb = i, 200 + (i + 7) % 200
        if swap:
            ka, kb = kb, ka
    col = (i + n * rnd) % 400
    assert np.unique(col).size == n and np.unique(np.concatenate([ka, kb])).size == 2 * n

    V = 1 + D
    emb = np.zeros((V, K), np.float32)
    ids = np.zeros((n, F), np.int32)
    ra, rb = 1 + 2 * i, 2 + 2 * i
    emb[ra, pa % K] = pr.xa
    emb[rb, pb % K] = pr.xb
    ids[i, pa // K] = ra
    ids[i, pb // K] = rb

    offs, wo_off = _offsets()
    mats = np.zeros(N_MATS, np.float32)
    W = [mats[w:b].reshape(-1, dim) for (w, b, dim) in offs]
    bs = [mats[b:b + 400] for (w, b, dim) in offs]

    def put(Wl, r, c, v):
        assert np.all(Wl[r, c] == 0), "two samples collide in a weight entry"
        Wl[r, c] = v

    # selection layers before the probed one: layer-1 column ka / kb, then the identity
    if layer >= 2:
        put(W[0], ka, pa, 1.0)
        put(W[0], kb, pb, 1.0)
    if layer == 3:
        put(W[1], ka, ka, 1.0)
        put(W[1], kb, kb, 1.0)
    put(W[layer - 1], col, ka, pr.wa)
    put(W[layer - 1], col, kb, pr.wb)
    bs[layer - 1][col] = pr.b
    # gain: 2^10 per later layer, the rest of 2^e in the output weight
    for l in range(layer, 3):
        put(W[l], col, col, 2.0 ** 10)
    mats[wo_off + col] = 2.0 ** (pr.e - 10 * (3 - layer))
    mats[wo_off + 400] = B_OUT

    r = np.arange(B)
    sample = (r + 5 * (r // n)) % n  # repeats rotated: each probe meets other rows of a wave and of a block
    meta = dict(probe=probe, layer=layer, round=rnd, sample=sample, pos=np.stack([pa, pb], 1)[sample],
                kpos=np.stack([ka, kb], 1)[sample], col=col[sample])
    logit = np.full(B, pr.kept + B_OUT + BETA, np.float64)
    return ProbeRound(V, np.zeros(V, np.float32), emb, np.ascontiguousarray(ids[sample]), mats,
                      np.array([BETA], np.float32), logit, meta)


def all_rounds():
    return [(p, l, r) for p in PROBES for l in LAYERS for r in range(ROUNDS)]


def gathered(rd):
    """(index, weights, embeddings) of a round: the reference contract's already-gathered host arrays."""
    B = rd.ids.shape[0]
    flat = rd.ids.ravel()
    return np.repeat(np.arange(B, dtype=np.int64), F), rd.w_table[flat], rd.emb_table[flat].ravel()


def describe(rd, bad, got, want, limit=6):
    """The first few mismatching rows of a probe round, for an assertion message."""
    m = rd.meta
    lines = ["probe %s, layer %d, round %d: %d of %d rows off" % (m["probe"], m["layer"], m["round"], bad.size,
                                                                   got.size)]
    for r in bad[:limit]:
        lines.append("  row %d (sample %d): input positions %s, layer-%d K positions %s, column %d: p = %.9g, "
                     "expected %.9g" % (r, m["sample"][r], m["pos"][r].tolist(), m["layer"], m["kpos"][r].tolist(),
                                        m["col"][r], got[r], want[r]))
    return "\n".join(lines)


# ------------------------------------------------------------- emulation ----
def split_linear(keep, only=None):
    """ref_numpy._linear with both operands split into three bf16 parts (round to nearest even, of the fp32
    values) and only the part products in `keep` summed (fp64: each product of two bf16 values is exact).
    only = n: the n-th split Linear called (1-based, one closure per forward) sums `keep`, the others all six."""
    keep = tuple(keep)
    assert set(keep) <= set(PRODUCTS6 + ("ml", "lm", "ll"))
    calls = [0]

    def lin(x, Wb):
        W, b = Wb
        if W.shape[0] == 1:  # the output head: a dot in plain fp32 on the device, not a split GEMM
            return ref_numpy._linear(x, Wb)
        calls[0] += 1
        prods = keep if only is None or calls[0] == only else PRODUCTS6
        xs = dict(zip("hml", (p.astype(np.float64) for p in split3(np.asarray(x, np.float32)))))
        ws = dict(zip("hml", (p.astype(np.float64) for p in split3(np.asarray(W, np.float32)))))
        y = 0.0
        for p in prods:
            y = y + ref_numpy._linear(xs[p[0]], (ws[p[1]], None))
        return y + b if b is not None else y

    return lin


@contextlib.contextmanager
def _patched_linear(fn):
    old = ref_numpy._linear

    def dispatch(x, Wb):
        ref_numpy._linear = old  # fn itself sums plain _linear calls
        try:
            return fn(x, Wb)
        finally:
            ref_numpy._linear = dispatch

    ref_numpy._linear = dispatch
    try:
        yield
    finally:
        ref_numpy._linear = old


def forward_split(keep, kind, B, Fn, k, index, bias, weights, emb, mats, only=None, **kw):
    """ref_numpy.forward with every Linear of the tower / CIN / product layers run by split_linear(keep);
    the first order, the FM, the cross layers and the one-column output Linear stay fp64.  Returns p in fp64."""
    with _patched_linear(split_linear(keep, only)):
        return ref_numpy.forward(kind, B, Fn, k, index, bias, weights, emb, mats, **kw)
