"""Helpers shared by the backward tests (test_train.py, test_shape_sweep*.py): the gradient bar against the
f64 oracle and the ReLU-tie filter of the rows a backward is compared on."""
import numpy as np


def _close(got, ref, rel=2e-5, rtol=1e-3, floor=1e-3):
    """fp32 device vs f64 oracle, two bars:
    max |got - ref| <= rel * max |ref|  (the whole array), and element by element
    |got - ref| <= rtol * max(|ref|, floor * max |ref|)  -- so small entries are held to 1e-6 of the
    largest one (20x the array-wide bar) and entries above the floor to 0.1 % of themselves."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    mx = max(float(np.abs(ref).max()), 1e-6)
    err = float(np.abs(got - ref).max()) / mx
    bound = rtol * np.maximum(np.abs(ref), floor * mx)
    bad = int((np.abs(got - ref) > bound).sum())
    if err > rel or bad:
        print("relative-to-max error %.3g (bar %.3g); %d entries over the element-wise bar" % (err, rel, bad))
    return err <= rel and bad == 0


def _hidden_pre(kind, E, mats, fc, cross=0, cin=()):
    """f64 pre-activations of every ReLU layer (rows = samples) of a tower-bearing model.
    cross: DCN's cross depth (its vectors and scalars precede the tower in mats); cin: xDeepFM's CIN maps."""
    B, F, k = E.shape
    D = F * k
    mats = np.asarray(mats, np.float64)
    x = E.reshape(B, D)
    pres, off = [], 0
    if kind == "dcn":
        off = cross * D + cross
    if kind == "pnn":
        rows = [i for i in range(F) for j in range(i + 1, F)]
        cols = [j for i in range(F) for j in range(i + 1, F)]
        ip = (E[:, rows] * E[:, cols]).sum(2)
        P, D1 = len(rows), fc[0]
        pre = x @ mats[:D * D1].reshape(D1, D).T + ip @ mats[D * D1:(D + P) * D1].reshape(D1, P).T + mats[(D + P) * D1]
        pres.append(pre)
        x, off, fc = np.maximum(pre, 0), (D + P) * D1 + 1, fc[1:]
    for d in fc:
        K_ = x.shape[1]
        pre = x @ mats[off:off + K_ * d].reshape(d, K_).T + mats[off + K_ * d:off + K_ * d + d]
        pres.append(pre)
        x, off = np.maximum(pre, 0), off + K_ * d + d
    if kind == "xdeepfm":  # CIN maps, rows (b, j) regrouped per sample
        x0 = E.transpose(0, 2, 1).reshape(B * k, F)
        u, hp = x0, F
        for h in cin:
            Z = (x0[:, :, None] * u[:, None, :]).reshape(B * k, F * hp)
            pre = Z @ mats[off:off + F * hp * h].reshape(h, F * hp).T + mats[off + F * hp * h:off + F * hp * h + h]
            pres.append(pre.reshape(B, k * h))
            u, off, hp = np.maximum(pre, 0), off + F * hp * h + h, h
    return pres


def _tie_free(kind, E, mats, fc, rel=1e-5, cross=0, cin=()):
    """Rows whose ReLU inputs all stay clear of zero: a pre-activation within fp32 rounding of 0 makes
    the ReLU mask ill-conditioned, and fp32 (device) and f64 (oracle) may then legitimately take
    different branches (observed: one row of 512 with pre = -1e-8, |pre| / mean 6e-7)."""
    ok = np.ones(E.shape[0], bool)
    for pre in _hidden_pre(kind, E, mats, fc, cross, cin):
        ok &= (np.abs(pre) > rel * np.abs(pre).mean()).all(axis=1)
    return np.where(ok)[0]
