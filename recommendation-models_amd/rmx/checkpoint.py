"""Checkpoints of the device-resident parameters: save / load of a model's mats and bias, a table's or a sharded
table's rows and an optimiser's state and step count, over the row upload / download calls (include/rmx.h
"loading and saving parameters").

A checkpoint is a directory of plain .npy files, opened as memmaps, plus one small meta.json:

    weights [V]   embedding [V][k]   mats [mats_len]   bias [1]
    s<slot>_weights [V]   s<slot>_embedding [V][k]   s<slot>_mats [mats_len]   s<slot>_bias [1]   (per state slot)
    meta.json: V, k, the model's kind and dims, the optimiser's kind, hyper-parameters and steps

The arrays are indexed by GLOBAL id, so a checkpoint does not depend on the number of ranks or on the owner key:
one saved from a 2-rank shard loads into a 3-rank one, or into a replicated table.  Rows move chunk by chunk
(chunk_rows at a time): save never holds more than one chunk in host memory.

Several ranks: every rank of a multi-rank shard calls save() with the same path and writes only the rows it owns
into the shared memmaps; the replicated parts (mats, bias, their state, meta.json) are written by rank 0.  The
files must exist before a rank other than 0 writes: call prepare() once first, then save() on every rank
(create defaults to True on rank 0 and on anything that is not a multi-rank shard; after prepare() pass False).
On load every rank reads every chunk and keeps its own rows.
"""
import json
import os

import numpy as np

FORMAT = 1
MODEL_LR, MODEL_DNN = 0, 5


def _layout(model, table, optim):
    """The meta dictionary and {array name: shape} of a checkpoint of these objects."""
    V, k = int(table.rows), int(table.k)
    input_dim, n_fields, kk, fc, cin, depth = model._args
    meta = {"format": FORMAT, "V": V, "k": k,
            "model": {"kind": int(model._kind), "inputDim": input_dim, "nFields": n_fields, "embeddingDim": kk,
                      "fcDims": list(fc), "cinDims": list(cin), "crossDepth": depth},
            "optimizer": None}
    ml = int(model.matsLength())
    shapes = {"weights": (V,), "mats": (ml,), "bias": (1,)}
    if k > 0:
        shapes["embedding"] = (V, k)
    if optim is not None:
        has_w = model._kind != MODEL_DNN
        has_e = model._kind != MODEL_LR and k > 0
        meta["optimizer"] = {"kind": int(optim.kind), "hyper": dict(optim.hyper), "steps": int(optim.steps),
                             "slots": int(optim.nslots), "weights": has_w, "embedding": has_e}
        for s in range(optim.nslots):
            if has_w:
                shapes["s%d_weights" % s] = (V,)
            if has_e:
                shapes["s%d_embedding" % s] = (V, k)
            shapes["s%d_mats" % s] = (ml,)
            shapes["s%d_bias" % s] = (1,)
    return meta, shapes


def _file(path, name):
    return os.path.join(path, name + ".npy")


def _open(path, name, shape, mode):
    if 0 in shape:  # (a memmap cannot be empty)
        return np.zeros(shape, np.float32)
    if mode == "w+":
        return np.lib.format.open_memmap(_file(path, name), mode="w+", dtype=np.float32, shape=shape)
    a = np.load(_file(path, name), mmap_mode=mode)
    if a.shape != tuple(shape) or a.dtype != np.float32:
        raise ValueError("checkpoint array %s is %s %s, expected float32 %s" % (name, a.dtype, a.shape, shape))
    return a


def _write_meta(path, meta):
    tmp = os.path.join(path, "meta.json.tmp")
    with open(tmp, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    os.replace(tmp, os.path.join(path, "meta.json"))


def read_meta(path):
    with open(os.path.join(path, "meta.json")) as f:
        return json.load(f)


def prepare(path, model, table, optim=None):
    """Create the checkpoint directory with zero-filled arrays and meta.json (steps as they are now).  Needed on
    its own only before the ranks of a multi-rank shard save into it."""
    os.makedirs(path, exist_ok=True)
    meta, shapes = _layout(model, table, optim)
    for name, shape in shapes.items():
        a = _open(path, name, shape, "w+")
        if isinstance(a, np.memmap):
            a.flush()
        del a
    _write_meta(path, meta)
    return meta


def check_meta(meta, model, table, optim=None):
    """Raise ValueError unless the checkpoint described by meta fits these objects (V, k, the model's kind and
    dims, the optimiser's kind).  Touches no device."""
    want, _ = _layout(model, table, None)
    if meta.get("format") != FORMAT:
        raise ValueError("checkpoint format %r, this library reads %d" % (meta.get("format"), FORMAT))
    for key in ("V", "k"):
        if meta.get(key) != want[key]:
            raise ValueError("checkpoint %s = %r, the table has %r" % (key, meta.get(key), want[key]))
    for key, val in want["model"].items():
        if meta.get("model", {}).get(key) != val:
            raise ValueError("checkpoint model %s = %r, the model has %r" % (key, meta.get("model", {}).get(key), val))
    if optim is not None:
        mo = meta.get("optimizer")
        if not mo:
            raise ValueError("the checkpoint holds no optimiser state")
        if mo.get("kind") != int(optim.kind):
            raise ValueError("checkpoint optimiser kind %r, the optimiser is kind %d" % (mo.get("kind"), optim.kind))


def _multi_rank(table):
    return getattr(table, "nranks", 1) > 1 and not getattr(table, "loopback", False)


def _put(dst, i0, src, owned):
    """dst[i0 : i0 + n] = src, the owned rows only."""
    n = len(src)
    if owned is None or owned.all():
        dst[i0:i0 + n] = src
    elif owned.any():
        dst[i0:i0 + n][owned] = src[owned]


def save(path, model, table, optim=None, chunk_rows=1 << 18, create=None):
    """Write the parameters (and, with optim, the optimiser's state and step count) to directory `path`.
    table: an EmbeddingTable or a ShardedTable; every rank of a multi-rank shard calls save() and writes the
    rows it owns (see the module docstring for who creates the files)."""
    multi = _multi_rank(table)
    lead = not multi or table.rank == 0
    if create is None:
        create = lead
    meta, shapes = _layout(model, table, optim)
    if create:
        prepare(path, model, table, optim)
    else:
        check_meta(read_meta(path), model, table, optim)
    arrs = {name: _open(path, name, shape, "r+") for name, shape in shapes.items()}
    V, k = meta["V"], meta["k"]
    sharded = hasattr(table, "nranks")
    chunk_rows = max(int(chunk_rows), 1)
    mo = meta["optimizer"]
    for i0 in range(0, V, chunk_rows):
        n = min(chunk_rows, V - i0)
        res = table.download_rows(i0, n)
        owned = res[2] if sharded else None
        _put(arrs["weights"], i0, res[0], owned)
        if k > 0:
            _put(arrs["embedding"], i0, res[1], owned)
        for s in range(mo["slots"] if mo else 0):
            w, e, own = optim.state_download_rows(s, i0, n, want_weights=mo["weights"], want_embedding=mo["embedding"])
            own = own if sharded else None
            if mo["weights"]:
                _put(arrs["s%d_weights" % s], i0, w, own)
            if mo["embedding"]:
                _put(arrs["s%d_embedding" % s], i0, e, own)
    if lead:
        if arrs["mats"].size:
            arrs["mats"][:] = model.getMats()
        arrs["bias"][0] = model.getBias()
        for s in range(mo["slots"] if mo else 0):
            m, b = optim.state_download_dense(s)
            if m.size:
                arrs["s%d_mats" % s][:] = m
            arrs["s%d_bias" % s][0] = b
        _write_meta(path, meta)
    for a in arrs.values():
        if isinstance(a, np.memmap):
            a.flush()
    return meta


def load(path, model, table, optim=None, chunk_rows=1 << 18):
    """Restore what save() wrote into these objects: mats and bias into the model, the rows into the table (every
    rank of a shard reads every chunk and keeps its own rows), and with optim its state and step count.  A
    checkpoint of another V, k, model kind or dims, or optimiser kind raises ValueError before anything is written
    to the device."""
    meta = read_meta(path)
    check_meta(meta, model, table, optim)
    _, shapes = _layout(model, table, optim)
    arrs = {name: _open(path, name, shape, "r") for name, shape in shapes.items()}  # (shape mismatches raise here)
    V, k = meta["V"], meta["k"]
    mo = meta["optimizer"] if optim is not None else None
    if arrs["mats"].size or model.matsLength() == 0:
        model.setMats(np.asarray(arrs["mats"]))
    model.setBias(float(arrs["bias"][0]))
    chunk_rows = max(int(chunk_rows), 1)
    for i0 in range(0, V, chunk_rows):
        n = min(chunk_rows, V - i0)
        table.upload_rows(i0, arrs["weights"][i0:i0 + n], arrs["embedding"][i0:i0 + n] if k > 0 else None)
        for s in range(mo["slots"] if mo else 0):
            optim.state_upload_rows(s, i0,
                                    arrs["s%d_weights" % s][i0:i0 + n] if mo["weights"] else None,
                                    arrs["s%d_embedding" % s][i0:i0 + n] if mo["embedding"] else None)
    if mo:
        for s in range(mo["slots"]):
            optim.state_upload_dense(s, np.asarray(arrs["s%d_mats" % s]) if arrs["s%d_mats" % s].size else None,
                                     float(arrs["s%d_bias" % s][0]))
        optim.steps = int(mo["steps"])
    return meta


__all__ = ["save", "load", "prepare", "check_meta", "read_meta"]
