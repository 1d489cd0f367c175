"""The parts of parameter loading and saving that need no GPU: the argument checks that come before any device
call (include/rmx.h "loading and saving parameters") and the checkpoint layout (rmx/checkpoint.py) on numpy
stand-ins for the table and the optimiser.  Nothing here makes a device call."""
import ctypes
import json
import os

import numpy as np
import pytest

import rmx
from rmx import _lib, checkpoint

L = _lib.lib
INV = _lib.RMX_E_INVALID
ROW_CALLS = [
    ("rmx_table_upload_rows", lambda n, lay, ld: (None, 0, n, None, None, lay, ld)),
    ("rmx_table_download_rows", lambda n, lay, ld: (None, 0, n, None, None, lay, ld)),
    ("rmx_shard_upload_rows", lambda n, lay, ld: (None, 0, n, None, None, lay, ld, None)),
    ("rmx_shard_download_rows", lambda n, lay, ld: (None, 0, n, None, None, lay, ld, None, None)),
    ("rmx_optim_state_upload_rows", lambda n, lay, ld: (None, 0, 0, n, None, None, lay, ld, None)),
    ("rmx_optim_state_download_rows", lambda n, lay, ld: (None, 0, 0, n, None, None, lay, ld, None, None)),
]


def _err():
    return (L.rmx_last_error() or b"").decode()


@pytest.mark.parametrize("name,args", ROW_CALLS, ids=[c[0] for c in ROW_CALLS])
def test_null_handles_return_invalid_whatever_the_range(name, args):
    """A NULL handle is RMX_E_INVALID before anything else is looked at, with good and with bad ranges alike (the
    n, layout, ld and range branches need a live handle: tests/test_param_io.py covers them on the GPU)."""
    fn = getattr(L, name)
    for n, lay, ld in ((8, _lib.LAYOUT_ROW_MAJOR, 0), (0, _lib.LAYOUT_ROW_MAJOR, 0), (-3, _lib.LAYOUT_K_MAJOR, 1),
                       (8, 9, 0), (8, _lib.LAYOUT_K_MAJOR, 2)):
        assert fn(*args(n, lay, ld)) == INV, (name, n, lay, ld)
        assert name in _err() and "NULL" in _err()


def test_null_kernel_hooks():
    for fn in (L.rmx_debug_table_row_kernels, L.rmx_debug_shard_row_kernels):
        assert fn(None, 0, 8, 1, _lib.LAYOUT_ROW_MAJOR, None, None) == INV and "NULL" in _err()


def test_null_optimiser_calls():
    one = np.zeros(1, np.float32)
    p = ctypes.c_void_p(one.ctypes.data)
    assert L.rmx_optim_state_upload_dense(None, 0, None, p) == INV and "NULL" in _err()
    assert L.rmx_optim_state_download_dense(None, 0, None, p) == INV and "NULL" in _err()
    assert L.rmx_optim_set_steps(None, 3) == INV and "NULL" in _err()
    assert one[0] == 0


def test_the_knob_is_plain_tuning():
    assert rmx.get_tuning("io_chunk_rows", -1) == -1
    rmx.set_tuning("io_chunk_rows", 4096)
    assert rmx.get_tuning("io_chunk_rows", -1) == 4096
    rmx.set_tuning("io_chunk_rows", None)
    assert rmx.get_tuning("io_chunk_rows", -1) == -1


# ------------------------------------------------------------------ checkpoint layout on numpy stand-ins ----
V, K, F, FC = 1003, 4, 3, [8, 4]


class HostTable:
    """The row interface of EmbeddingTable over numpy arrays."""

    def __init__(self, rows, k, seed=None):
        self.rows, self.k = rows, k
        rng = np.random.default_rng(seed)
        self.w = np.zeros(rows, np.float32) if seed is None else rng.normal(0, 1, rows).astype(np.float32)
        self.e = np.zeros((rows, k), np.float32) if seed is None else rng.normal(0, 1, (rows, k)).astype(np.float32)
        self.calls = []

    def download_rows(self, id0, n):
        self.calls.append(n)
        return self.w[id0:id0 + n].copy(), self.e[id0:id0 + n].copy()

    def upload_rows(self, id0, weights=None, embedding=None):
        self.calls.append(len(weights))
        self.w[id0:id0 + len(weights)] = weights
        self.e[id0:id0 + len(embedding)] = embedding


class HostShard(HostTable):
    """Rank `rank` of `nranks`: owns the ids with id % nranks == rank, returns garbage for the others."""

    def __init__(self, rows, k, nranks, rank, seed=None):
        super().__init__(rows, k, seed)
        self.nranks, self.rank, self.loopback = nranks, rank, False
        self.own = np.arange(rows) % nranks == rank

    def download_rows(self, id0, n):
        w, e = super().download_rows(id0, n)
        own = self.own[id0:id0 + n]
        w[~own], e[~own] = np.nan, np.nan
        return w, e, own


class HostModel:
    _kind = 1  # DeepFM

    def __init__(self, fc=FC, seed=None):
        self._args = (V, F, K, tuple(fc), (), 0)
        self.n = sum(fc) * 3 + 7
        self.mats = (np.zeros(self.n, np.float32) if seed is None
                     else np.random.default_rng(seed).normal(0, 1, self.n).astype(np.float32))
        self.bias = 0.0 if seed is None else 0.25

    def matsLength(self):
        return self.n

    def getMats(self):
        return self.mats.copy()

    def getBias(self):
        return self.bias

    def setMats(self, m):
        self.mats = np.array(m, np.float32)

    def setBias(self, b):
        self.bias = float(b)


class HostOptim:
    kind, nslots = 3, 2

    def __init__(self, model, seed=None):
        self.hyper = {"eta": 0.01, "gamma": 0.99, "beta": 0.9, "eps": 1e-7}
        self.steps = 0 if seed is None else 17
        self.tabs = [HostTable(V, K, None if seed is None else seed + s) for s in range(2)]
        self.dense = [(model.getMats() * (s + 2), 0.5 * (s + 1) if seed is not None else 0.0) for s in range(2)]

    def state_download_rows(self, slot, id0, n, want_weights=True, want_embedding=True):
        w, e = self.tabs[slot].download_rows(id0, n)
        return w, e, np.ones(n, bool)

    def state_upload_rows(self, slot, id0, weights=None, embedding=None):
        self.tabs[slot].upload_rows(id0, weights, embedding)

    def state_download_dense(self, slot):
        return self.dense[slot]

    def state_upload_dense(self, slot, mats=None, bias=None):
        self.dense[slot] = (np.array(mats, np.float32), float(bias))


def test_checkpoint_layout_round_trip(tmp_path):
    path = str(tmp_path / "ck")
    model, table = HostModel(seed=1), HostTable(V, K, seed=2)
    opt = HostOptim(model, seed=3)
    checkpoint.save(path, model, table, opt, chunk_rows=100)
    assert max(table.calls) == 100 and len(table.calls) == 11  # chunk by chunk, a short last one
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["V"] == V and meta["k"] == K and meta["model"]["kind"] == 1 and meta["model"]["fcDims"] == FC
    assert meta["optimizer"]["kind"] == 3 and meta["optimizer"]["steps"] == 17
    assert meta["optimizer"]["hyper"]["gamma"] == 0.99
    names = sorted(f for f in os.listdir(path) if f.endswith(".npy"))
    assert names == sorted(["weights.npy", "embedding.npy", "mats.npy", "bias.npy"] +
                           ["s%d_%s.npy" % (s, p) for s in range(2) for p in ("weights", "embedding", "mats", "bias")])
    assert np.array_equal(np.load(os.path.join(path, "embedding.npy")), table.e)  # plain .npy, global-id indexed
    assert np.load(os.path.join(path, "s1_weights.npy")).shape == (V,)
    m2, t2 = HostModel(), HostTable(V, K)
    o2 = HostOptim(m2)
    checkpoint.load(path, m2, t2, o2, chunk_rows=64)
    assert np.array_equal(t2.w, table.w) and np.array_equal(t2.e, table.e)
    assert np.array_equal(m2.mats, model.mats) and m2.bias == model.bias and o2.steps == 17
    for s in range(2):
        assert np.array_equal(o2.tabs[s].w, opt.tabs[s].w) and np.array_equal(o2.tabs[s].e, opt.tabs[s].e)
        assert np.array_equal(o2.dense[s][0], opt.dense[s][0]) and o2.dense[s][1] == opt.dense[s][1]


def test_ranks_write_only_their_rows(tmp_path):
    path = str(tmp_path / "ck")
    model = HostModel(seed=1)
    shards = [HostShard(V, K, 2, r, seed=5) for r in range(2)]  # the same table, seen by two ranks
    checkpoint.prepare(path, model, shards[0])
    for sh in reversed(shards):
        checkpoint.save(path, model, sh, chunk_rows=333, create=False)
    got = np.load(os.path.join(path, "embedding.npy"))
    assert np.array_equal(got, shards[0].e) and not np.isnan(np.load(os.path.join(path, "weights.npy"))).any()
    t = HostTable(V, K)
    checkpoint.load(path, HostModel(), t)  # a checkpoint of a shard loads into a replicated table
    assert np.array_equal(t.e, shards[0].e)


def test_mismatches_raise_before_anything_is_written(tmp_path):
    path = str(tmp_path / "ck")
    model, table = HostModel(seed=1), HostTable(V, K, seed=2)
    checkpoint.save(path, model, table)

    def refused(m, t, o=None):
        t.calls.clear()
        before = (m.mats.copy(), m.bias)
        with pytest.raises(ValueError):
            checkpoint.load(path, m, t, o)
        assert not t.calls and np.array_equal(m.mats, before[0]) and m.bias == before[1]

    refused(HostModel(), HostTable(V + 1, K))             # V
    refused(HostModel(), HostTable(V, K + 1))             # k
    refused(HostModel(fc=[8, 5]), HostTable(V, K))        # dims
    lr = HostModel()
    lr._kind = 0
    refused(lr, HostTable(V, K))                          # kind
    refused(HostModel(), HostTable(V, K), HostOptim(HostModel()))  # no optimiser state in the checkpoint
    opt = HostOptim(model, seed=3)
    checkpoint.save(path, model, table, opt)
    sgd = HostOptim(HostModel())
    sgd.kind, sgd.nslots = 0, 0
    refused(HostModel(), HostTable(V, K), sgd)            # optimiser kind
    checkpoint.load(path, HostModel(), HostTable(V, K))   # the rows alone still load
