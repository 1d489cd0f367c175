"""numpy reference of the device optimiser step (include/rmx.h "optimiser") -- TEST INFRASTRUCTURE ONLY.

Formulas (g the aggregated gradient, t the step count, 1 on the first apply, the same for every group):
  sgd       p -= eta g
  momentum  v = momentum v + g;  p -= eta v
  adagrad   s = factor s + (1 - factor) g^2;  p -= eta g / (sqrt(s) + eps)
  adam      m = beta m + (1 - beta) g;  v = gamma v + (1 - gamma) g^2
            p -= eta (m / (1 - beta^t)) / (sqrt(v / (1 - gamma^t)) + eps)
Two modes: dtype=np.float64 (the formulas in double) and dtype=np.float32 (every operation rounded to fp32,
the constants 1 - a and 1 - a^t computed in double and rounded once, as the library does).

aggregate32 is the summation-order contract itself: an id's gradient is the sequential np.float32 sum of its
nonzeros' gradients in ascending nonzero order starting from the first term; a list of more than 512
occurrences is summed in consecutive chunks of 512 in that order, and the chunk sums are then added in chunk order.
"""
import numpy as np

KINDS = ("sgd", "momentum", "adagrad", "adam")
DEFAULTS = {
    "sgd": (("eta", None),),
    "momentum": (("eta", None), ("momentum", 0.9)),
    "adagrad": (("eta", None), ("factor", 0.9), ("eps", 1e-7)),
    "adam": (("eta", None), ("gamma", 0.99), ("beta", 0.9), ("eps", 1e-7)),
}
NSLOTS = {"sgd": 0, "momentum": 1, "adagrad": 1, "adam": 2}
CHUNK = 512


def hyper(kind, **kw):
    """The kind's hyper-parameters with the defaults filled in (eta has none)."""
    hp = {n: d for n, d in DEFAULTS[kind]}
    unknown = set(kw) - set(hp)
    if unknown:
        raise TypeError("%s takes no %s" % (kind, sorted(unknown)))
    hp.update(kw)
    if hp["eta"] is None:
        raise TypeError("eta is required")
    return hp


def radix_passes(V):
    """(bits, passes) of the device's id sort on a table of V rows (optim.hip id_bits, restated): the bits of the
    largest key -- V itself, the key given to an id outside the table -- and one 8-bit pass per started byte."""
    bits = 1
    while V >> bits:
        bits += 1
    return bits, (bits + 7) // 8


def _seq_sum32(rows, starts, counts):
    """Per list i: the sequential fp32 sum of rows[starts[i] : starts[i] + counts[i]] starting from the first
    term.  rows [n, c] float32; vectorised over the lists, sequential along each."""
    acc = rows[starts].astype(np.float32).copy()
    for r in range(1, int(counts.max()) if len(counts) else 0):
        sel = np.nonzero(counts > r)[0]
        acc[sel] = (acc[sel] + rows[starts[sel] + r]).astype(np.float32)
    return acc


def aggregate32(ids, g, V):
    """(distinct ids in [0, V) ascending, their gradient sums [n_distinct, c]) in the contract order.
    ids [nnz]; g [nnz] or [nnz, c] float32.  Ids outside [0, V) are skipped."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    g = np.ascontiguousarray(g, np.float32).reshape(len(ids), -1)
    keep = np.nonzero((ids >= 0) & (ids < V))[0]
    order = keep[np.argsort(ids[keep], kind="stable")]  # nonzeros grouped by id, ascending within an id
    sid = ids[order]
    rows = g[order]
    uniq, first, cnt = np.unique(sid, return_index=True, return_counts=True)
    if len(uniq) == 0:
        return uniq, np.zeros((0, g.shape[1]), np.float32)
    # chunks of at most 512 consecutive occurrences
    nch = (cnt + CHUNK - 1) // CHUNK
    owner = np.repeat(np.arange(len(uniq)), nch)
    cidx = np.arange(nch.sum()) - np.repeat(np.cumsum(nch) - nch, nch)
    cstart = first[owner] + cidx * CHUNK
    ccnt = np.minimum(CHUNK, cnt[owner] - cidx * CHUNK)
    csum = _seq_sum32(rows, cstart, ccnt)
    # the chunk sums of one id, added in chunk order
    total = _seq_sum32(csum, np.cumsum(nch) - nch, nch)
    return uniq, total


def aggregate64(ids, g, V):
    """The same sums in double (order immaterial at the tests' bars)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    g = np.asarray(g, np.float64).reshape(len(ids), -1)
    keep = (ids >= 0) & (ids < V)
    uniq, inv = np.unique(ids[keep], return_inverse=True)
    total = np.zeros((len(uniq), g.shape[1]), np.float64)
    np.add.at(total, inv, g[keep])
    return uniq, total


def update(kind, hp, p, g, slots, t, dtype=np.float64):
    """One step of `kind` on the parameters p with gradient g (same shape) at step count t.  slots: the list of
    NSLOTS[kind] state arrays.  Returns (new p, new slots); nothing is changed in place."""
    f = dtype
    p = np.asarray(p, f)
    g = np.asarray(g, f)
    eta = f(hp["eta"])
    if kind == "sgd":
        return (p - eta * g).astype(f), []
    if kind == "momentum":
        v = (f(hp["momentum"]) * np.asarray(slots[0], f) + g).astype(f)
        return (p - eta * v).astype(f), [v]
    if kind == "adagrad":
        fa = hp["factor"]
        s = (f(fa) * np.asarray(slots[0], f) + f(1.0 - fa) * (g * g).astype(f)).astype(f)
        return (p - (eta * g).astype(f) / (np.sqrt(s).astype(f) + f(hp["eps"]))).astype(f), [s]
    if kind == "adam":
        be, ga = hp["beta"], hp["gamma"]
        m = (f(be) * np.asarray(slots[0], f) + f(1.0 - be) * g).astype(f)
        v = (f(ga) * np.asarray(slots[1], f) + f(1.0 - ga) * (g * g).astype(f)).astype(f)
        c1, c2 = f(1.0 - be ** t), f(1.0 - ga ** t)
        mh = (m / c1).astype(f)
        vh = (v / c2).astype(f)
        return (p - (eta * mh).astype(f) / (np.sqrt(vh).astype(f) + f(hp["eps"]))).astype(f), [m, v]
    raise ValueError(kind)


class RefOptim:
    """The optimiser over one (table, mats, bias) set.  w [V], emb [V, k], mats [n], bias scalar; any may be None
    (group absent: LR has no emb / mats, DNN no w).  The sparse groups are always aggregated in the fp32
    contract order; the formulas then run in `dtype`."""

    def __init__(self, kind, hp, w=None, emb=None, mats=None, bias=0.0, dtype=np.float64):
        self.kind, self.hp, self.dtype = kind, hp, dtype
        self.t = 0
        cp = lambda a: None if a is None else np.array(a, dtype)
        self.w, self.emb, self.mats = cp(w), cp(emb), cp(mats)
        self.bias = np.array([bias], dtype)
        n = NSLOTS[kind]
        zl = lambda a: None if a is None else [np.zeros_like(a) for _ in range(n)]
        self.s_w, self.s_emb, self.s_mats, self.s_bias = zl(self.w), zl(self.emb), zl(self.mats), zl(self.bias)

    def _sparse(self, arr, slots, ids, g):
        V = arr.shape[0]
        uniq, gs = aggregate32(ids, g, V)
        if len(uniq) == 0:
            return
        rows = arr.reshape(V, -1)
        new, ns = update(self.kind, self.hp, rows[uniq], gs, [s.reshape(V, -1)[uniq] for s in slots], self.t,
                         self.dtype)
        rows[uniq] = new
        for s, v in zip(slots, ns):
            s.reshape(V, -1)[uniq] = v

    def apply(self, ids, g_bias=None, g_w=None, g_emb=None, g_mats=None):
        self.t += 1
        if g_w is not None and self.w is not None:
            self._sparse(self.w, self.s_w, ids, g_w)
        if g_emb is not None and self.emb is not None:
            self._sparse(self.emb, self.s_emb, ids, g_emb)
        if g_mats is not None and self.mats is not None:
            self.mats, self.s_mats = update(self.kind, self.hp, self.mats, np.asarray(g_mats, np.float32), self.s_mats,
                                            self.t, self.dtype)
        if g_bias is not None:
            self.bias, self.s_bias = update(self.kind, self.hp, self.bias, np.asarray(g_bias, np.float32).reshape(1),
                                            self.s_bias, self.t, self.dtype)
