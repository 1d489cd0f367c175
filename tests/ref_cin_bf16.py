"""numpy restatement of the xDeepFM forward with a bf16 CIN, and the exact probe networks of its tests --
TEST INFRASTRUCTURE ONLY.

rmx_model_set_cin_precision(RMX_DTYPE_BF16) (include/rmx.h) has exactly two storage points:
    weights   C_l rounded to bf16 (nearest even), element by element as given in mats;
    operand   z[r][f Hp + h] = bf16_rne(fl32(x0[r][f] * u_{l-1}[r][h])).
Everything else is fp32 on the device: accumulation, bias, ReLU, the maps u_l kept between layers, the pooled
sums and the output Linear.  forward() is ref_numpy.forward's xdeepfm branch (CINEncoder.scala:36-58, 105-176)
with those two roundings and u cast to fp32 after the ReLU.  Switches:
    acc = "fp64"  the K sums in fp64 -- THE REFERENCE;
    acc = "fp32"  an fp32 accumulator over 32-wide K steps (each step's 32 products summed exactly, one fp32
                  rounding per step, as the MFMA accumulates): used only for clearances;
    round_z = "trunc"  z cut toward zero instead of rounded: the nearest wrong arithmetic, used only for the bar;
    round_z = None, round_w = False: no rounding at all -- then it equals ref_numpy.forward to fp64 round-off.
The CIN's z rows are [rows 16][F Hp] doubles: callers pass at most 64 rows (rows_of).
"""
import numpy as np

import oracle_ctypes as oc
import ref_numpy
from ref_numpy import Mats, _relu, _sigmoid

MAX_ROWS = 64


def rows_of(B, n=MAX_ROWS):
    """At most n rows of a batch: its head, middle and tail."""
    if B <= n:
        return np.arange(B)
    a = n // 3
    return np.concatenate([np.arange(n - 2 * a), B // 2 - a // 2 + np.arange(a), B - a + np.arange(a)])


def trunc_bf16(x):
    """fp32 -> bf16 toward zero (the low 16 bits cut), as fp32."""
    x = np.ascontiguousarray(x, np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _rz(z32, mode):
    if mode == "rne":
        return oc.round_bf16(z32)
    if mode == "trunc":
        return trunc_bf16(z32)
    raise ValueError(mode)


def _gemm(Z, W, acc):
    """Z [M][K] x W [N][K]^T: fp64, or an fp32 accumulator over 32-wide K steps."""
    if acc == "fp64":
        return Z @ W.T
    assert acc == "fp32"
    a = np.zeros((Z.shape[0], W.shape[0]), np.float32)
    for s in range(0, Z.shape[1], 32):
        a = (a.astype(np.float64) + Z[:, s:s + 32] @ W[:, s:s + 32].T).astype(np.float32)
    return a.astype(np.float64)


def forward(B, F, k, index, bias, weights, emb, mats_flat, fc, cin, round_w=True, round_z="rne", acc="fp64",
            detail=None):
    """p [B] (fp64) of an xDeepFM.  detail: a dict that receives z (list per layer, fp64), w (the weights used),
    u (per layer), pools and logit."""
    exact = not round_w and round_z is None  # the unrounded model: everything in fp64, as ref_numpy
    bias = float(np.asarray(bias).reshape(-1)[0])
    mats = Mats(mats_flat)
    E = np.asarray(emb, np.float64)
    d = ref_numpy.tower(E.reshape(B, F * k), mats, fc, False)
    y1 = ref_numpy.scatter(B, index, weights)
    x0 = E.reshape(B, F, k).transpose(0, 2, 1).reshape(B * k, F)
    u = x0
    pools, hp = [], F
    zs, ws, us = [], [], []
    for h in cin:
        W, b = mats.linear(F * hp, h, True)
        if round_w:
            W = oc.round_bf16(W.astype(np.float32)).astype(np.float64)
        if round_z is None:
            Z = (x0[:, :, None] * u[:, None, :]).reshape(B * k, F * hp)
        else:  # one fp32 multiply, then one rounding to bf16
            z32 = (x0.astype(np.float32)[:, :, None] * u.astype(np.float32)[:, None, :]).reshape(B * k, F * hp)
            Z = _rz(z32, round_z).astype(np.float64)
        pre = _gemm(Z, W, acc)
        if acc == "fp32":
            pre = (pre.astype(np.float32) + b.astype(np.float32)).astype(np.float64)
        else:
            pre = pre + b
        u = _relu(pre)
        if not exact:
            u = u.astype(np.float32).astype(np.float64)  # the maps are stored fp32 between layers
        pools.append(u.reshape(B, k, h).sum(axis=1))
        zs.append(Z)
        ws.append(W)
        us.append(u)
        hp = h
    Wo, _ = mats.linear(sum(cin) + fc[-1], 1, False)
    y = np.concatenate(pools + [d], axis=1) @ Wo.T
    logit = (y1 + y[:, 0]) + bias
    if detail is not None:
        detail.update(z=zs, w=ws, u=us, pools=pools, logit=logit)
    return _sigmoid(logit)


def logit(p):
    p = np.asarray(p, np.float64)
    return np.log(p / (1.0 - p))


# ------------------------------------------------------------------ exact probes ----
# Inputs that make the bf16 CIN exact: every z and every weight is a bf16 value, every partial sum in any order
# is exact in fp32, so the device must return the bits of the fp64 evaluation -- a dropped or misplaced K chunk,
# a wrong field, pad or plane shows as a changed bit.  Table rows are in {0, +-0.5, +-1}; first-order weights,
# the tower and its output slice are zero: only the CIN reaches the logit.
#   probe A (one CIN layer):  C_1 dense in {-1, 0, 1} / 64, biases multiples of 1/8;
#   probe B (two):            C_1 two entries of +-0.5 per map (u_1 a multiple of 1/8 below 2: 4 significant bits,
#                             so z_2 = x0 u_1 is a bf16 value), biases multiples of 1/8; C_2 dense in
#                             {-1, 0, 1} / 128, biases multiples of 1/256.
# The CIN output weights are PER_ROUND entries of +-2^-n per round, rotated so that every map is read once.
PROBE_V = 257
PROBE_FC = (16,)
PROBE_BETA = 0.125
PROBE_SHAPES = ((39, (200,)), (39, (200, 200)), (5, (200, 7)), (5, (10, 7)), (17, (256, 3)), (41, (5,)))
PER_ROUND = 32
# batches: one partial block, ragged blocks, and one per tile of the selection (cin_bf16_tiles)
PROBE_BATCHES = (37, 517, 1100, 4099)


def probe_table():
    rng = np.random.default_rng(0xC1B)
    emb = rng.choice(np.array([0.0, 0.5, -0.5, 1.0, -1.0], np.float32), size=(PROBE_V, 16))
    return np.zeros(PROBE_V, np.float32), np.ascontiguousarray(emb, np.float32)


def probe_ids(F, B):
    return np.random.default_rng(1000 + F).integers(0, PROBE_V, size=(B, F)).astype(np.int32)


def probe_layout(F, cin):
    """Offsets in mats: [(C offset, bias offset, Hp, H)] per CIN layer, the CIN slice of W_out, the length."""
    off, prev = 0, F * 16
    for d_ in PROBE_FC:
        off += prev * d_ + d_
        prev = d_
    lay, hp = [], F
    for h in cin:
        lay.append((off, off + F * hp * h, hp, h))
        off += F * hp * h + h
        hp = h
    return lay, off, off + sum(cin) + PROBE_FC[-1]


def probe_rounds(cin):
    return -(-max(cin) // PER_ROUND)


def probe_mats(F, cin, rnd):
    """The mats of round rnd (the CIN weights and biases are the same in every round; W_out rotates)."""
    assert len(cin) in (1, 2)
    rng = np.random.default_rng(77 + 13 * F + sum(cin))
    lay, wo_off, n = probe_layout(F, cin)
    mats = np.zeros(n, np.float32)
    (c1, b1, hp1, h1) = lay[0]
    if len(cin) == 1:
        mats[c1:b1] = rng.integers(-1, 2, size=h1 * F * hp1) / 64.0
    else:
        C1 = mats[c1:b1].reshape(h1, F * hp1)
        for r in range(h1):
            cols = rng.choice(F * hp1, size=2, replace=False)
            C1[r, cols] = rng.choice([0.5, -0.5], size=2)
        (c2, b2, hp2, h2) = lay[1]
        mats[c2:b2] = rng.integers(-1, 2, size=h2 * F * hp2) / 128.0
        mats[b2:b2 + h2] = rng.integers(-4, 5, size=h2) / 256.0
    mats[b1:b1 + h1] = rng.integers(-2, 3, size=h1) / 8.0
    base = 0
    for (_, _, _, h) in lay:
        cols = np.arange(h)
        cols = cols[cols // PER_ROUND == rnd % -(-h // PER_ROUND)]
        sgn = np.where(cols % 2 == 0, 1.0, -1.0)  # maps 2i, 2i + 1: the same magnitude, opposite signs
        mats[wo_off + base + cols] = sgn * 2.0 ** -(4 + (cols // 2 + rnd) % 3)
        base += h
    return mats


def probe_expected(F, cin, ids, rnd, detail=None):
    """The exact logit (fp64) of rows ids [n][F] in round rnd."""
    wt, et = probe_table()
    n = ids.shape[0]
    flat = np.asarray(ids, np.int64).ravel()
    dt = {} if detail is None else detail
    forward(n, F, 16, np.repeat(np.arange(n, dtype=np.int64), F), np.array([PROBE_BETA], np.float32), wt[flat],
            et[flat].ravel(), probe_mats(F, cin, rnd), PROBE_FC, cin, detail=dt)
    return dt["logit"]


def sigmoid32(x):
    """sigmoid in fp64, rounded once to fp32 (split_probes.sigmoid32)."""
    return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))).astype(np.float32)


# ---------------------------------------------------------------- tile selection ----
NCU = 256


def cin_npad(H):
    nt = -(-H // 16)
    return 16 * next(c for c in (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 16) if c >= nt)


def cin_bf16_tiles(cin, B, k=16, ncu=NCU):
    """The tile each CIN layer runs on (k_cin_bf16.hip launch_cin_bf16_208 / launch_cin_bf16_nt), by M = B k."""
    M, out = B * k, []
    for h in cin:
        if cin_npad(h) == 208:
            blocks = lambda rows: -(-M // rows)
            out.append("ring_mt2_4w" if blocks(256) >= ncu else "ring_4w" if blocks(64) >= ncu else "ring_2w")
        else:
            out.append("plain_4w" if M < 8192 else "plain_mt2_8w")
    return out


ALL_TILES = ("ring_mt2_4w", "ring_4w", "ring_2w", "plain_4w", "plain_mt2_8w")
