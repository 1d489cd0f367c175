"""The optimiser's reference (tests/optim_ref.py) pinned against torch-CPU, the summation-order contract of its
fp32 aggregation, rmx_optim_create's argument checks on a host-only model, and the ctypes declarations of the new
entry points against include/rmx.h.  No GPU: nothing here makes a device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import optim_ref as R
import rmx
from rmx import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- formulas vs torch ----
def _torch_run(make_opt, p0, grads):
    import torch
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = make_opt(torch, [p])
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


TORCH_CASES = [
    ("sgd", dict(eta=0.05), lambda t, ps: t.optim.SGD(ps, lr=0.05)),
    ("momentum", dict(eta=0.05, momentum=0.9), lambda t, ps: t.optim.SGD(ps, lr=0.05, momentum=0.9)),
    ("momentum", dict(eta=0.02, momentum=0.5), lambda t, ps: t.optim.SGD(ps, lr=0.02, momentum=0.5)),
    ("adagrad", dict(eta=0.05, factor=0.9, eps=1e-7),
     lambda t, ps: t.optim.RMSprop(ps, lr=0.05, alpha=0.9, eps=1e-7)),
    ("adam", dict(eta=0.05, gamma=0.99, beta=0.9, eps=1e-7),
     lambda t, ps: t.optim.Adam(ps, lr=0.05, betas=(0.9, 0.99), eps=1e-7)),
]


@pytest.mark.parametrize("kind,hp,make_opt", TORCH_CASES, ids=[c[0] + str(i) for i, c in enumerate(TORCH_CASES)])
def test_dense_fp64_reference_equals_torch(kind, hp, make_opt):
    """5 steps of random gradients: the fp64 formulas equal torch.optim.SGD (plain / momentum), RMSprop (the
    Adagrad with a decay factor) and Adam to 1e-12 relative."""
    rng = np.random.default_rng(17)
    p0 = rng.normal(0, 0.1, 257)
    grads = [rng.normal(0, 1.0, 257) for _ in range(5)]
    want = _torch_run(make_opt, p0, grads)
    hp = R.hyper(kind, **hp)
    p, slots = p0.copy(), [np.zeros_like(p0) for _ in range(R.NSLOTS[kind])]
    for t, g in enumerate(grads, 1):
        p, slots = R.update(kind, hp, p, g, slots, t, np.float64)
        err = np.abs(p - want[t - 1]).max() / np.abs(want[t - 1]).max()
        assert err <= 1e-12, (kind, t, err)


def test_defaults_are_the_reference_constructor_defaults():
    assert R.hyper("momentum", eta=1.0)["momentum"] == 0.9
    assert R.hyper("adagrad", eta=1.0) == dict(eta=1.0, factor=0.9, eps=1e-7)
    assert R.hyper("adam", eta=1.0) == dict(eta=1.0, gamma=0.99, beta=0.9, eps=1e-7)
    assert rmx.Optimizer.HYPER[_lib.OPTIM_ADAM] == R.DEFAULTS["adam"]
    assert rmx.Optimizer.HYPER[_lib.OPTIM_ADAGRAD] == R.DEFAULTS["adagrad"]
    assert rmx.Optimizer.HYPER[_lib.OPTIM_MOMENTUM] == R.DEFAULTS["momentum"]


# ------------------------------------------------------------- aggregation contract ----
def test_aggregate32_is_the_sequential_sum_in_nonzero_order():
    """Against a plain loop: ascending nonzero order from the first term, 512-chunks for long lists, ids outside
    [0, V) skipped; and the fp32 result differs from a pairwise / fp64 sum (the order is visible)."""
    rng = np.random.default_rng(3)
    V, n, c = 50, 1400, 3
    ids = rng.integers(0, V, n)
    ids[::2] = 7          # 700+ occurrences: two chunks
    ids[5], ids[9] = -1, V
    g = (rng.normal(0, 1, (n, c)) * 10.0 ** rng.integers(-3, 3, (n, c))).astype(np.float32)
    uniq, tot = R.aggregate32(ids, g, V)
    assert uniq.tolist() == sorted(set(int(i) for i in ids if 0 <= i < V))
    for u, row in zip(uniq, tot):
        pos = np.nonzero(ids == u)[0]
        chunks = []
        for s in range(0, len(pos), 512):
            acc = g[pos[s]].copy()
            for q in pos[s + 1:s + 512]:
                acc = (acc + g[q]).astype(np.float32)
            chunks.append(acc)
        acc = chunks[0]
        for ch in chunks[1:]:
            acc = (acc + ch).astype(np.float32)
        assert np.array_equal(acc.view(np.uint32), row.view(np.uint32)), u
    u64, t64 = R.aggregate64(ids, g, V)
    assert np.array_equal(u64, uniq)
    assert np.abs(tot - t64).max() <= 1e-4 * np.abs(t64).max()
    assert np.any(tot != t64.astype(np.float32))


def test_reference_sparse_semantics():
    """Only rows whose id occurs in the batch change, parameters and state alike."""
    rng = np.random.default_rng(5)
    V, k = 40, 4
    w0, e0 = rng.normal(0, 1, V).astype(np.float32), rng.normal(0, 1, (V, k)).astype(np.float32)
    ids = np.array([3, 3, 9, 11, 3, 39])
    ref = R.RefOptim("adam", R.hyper("adam", eta=0.1), w0, e0, None, 0.5, np.float32)
    ref.apply(ids, g_bias=np.ones(1, np.float32), g_w=np.ones(6, np.float32), g_emb=np.ones((6, k), np.float32))
    touched = np.zeros(V, bool)
    touched[ids] = True
    assert np.array_equal(ref.w[~touched], w0[~touched]) and np.array_equal(ref.emb[~touched], e0[~touched])
    assert np.all(ref.w[touched] != w0[touched]) and np.all(ref.s_emb[0][touched] != 0)
    assert not ref.s_w[0][~touched].any() and not ref.s_emb[1][~touched].any()
    assert ref.bias[0] != 0.5 and ref.t == 1


def test_radix_passes_of_the_table_sizes_under_test():
    """The id sort's key width and pass count (optim.hip id_bits, (bits + 7) / 8) at the table sizes of
    test_optim.py: every V up to 5,003 of the other tests sorts in 2 passes; 255 is the last V of one pass, 65,536
    the first of three, 2^24 the first of four (the bench's V = 1,000,000 makes three)."""
    sizes = (255, 256, 65535, 65536, 16_777_300)
    assert [R.radix_passes(V) for V in sizes] == [(8, 1), (9, 2), (16, 2), (17, 3), (25, 4)]
    assert [R.radix_passes(V)[1] for V in (1, 2000, 5003, 1_000_000, (1 << 24) - 1, 1 << 24)] == [1, 2, 2, 3, 3, 4]
    for V in (255, 256, 65535, 65536, 16_777_300):
        bits, passes = R.radix_passes(V)
        assert V < 1 << bits and V >= 1 << (bits - 1)  # V, the key of an outside id, fits; no spare bit
        assert 8 * (passes - 1) < bits <= 8 * passes


# ------------------------------------------------------------ create's checks (host) ----
def _create(model_handle, table, kind, hyper, n=None):
    h = ctypes.c_void_p()
    arr = None if hyper is None else (ctypes.c_double * max(len(hyper), 1))(*hyper)
    st = _lib.lib.rmx_optim_create(model_handle, table, kind, arr, len(hyper or ()) if n is None else n,
                                   ctypes.byref(h))
    return st, (_lib.lib.rmx_last_error() or b"").decode(), h


def test_optim_create_argument_checks_on_a_host_only_model():
    """Every check of rmx_optim_create runs before any device call: a host-only model (no context, no GPU
    touched) reaches them all and fails RMX_E_INVALID with the reason."""
    m = rmx.DeepFM(2000, 39, 16, [24, 8])
    meta = m._meta
    inval = _lib.RMX_E_INVALID
    st, msg, _ = _create(None, None, _lib.OPTIM_SGD, [0.1])
    assert st == inval and "model is NULL" in msg
    assert _lib.lib.rmx_optim_create(meta, None, _lib.OPTIM_SGD, (ctypes.c_double * 1)(0.1), 1, None) == inval
    for kind in (-1, 4, 42):
        st, msg, _ = _create(meta, None, kind, [0.1])
        assert st == inval and "unknown optimiser kind" in msg
    st, msg, _ = _create(meta, None, _lib.OPTIM_SGD, None, 0)
    assert st == inval and "eta" in msg
    st, msg, _ = _create(meta, None, _lib.OPTIM_ADAM, [0.1], 0)
    assert st == inval and "eta" in msg
    for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
        for kind in (_lib.OPTIM_SGD, _lib.OPTIM_MOMENTUM, _lib.OPTIM_ADAGRAD, _lib.OPTIM_ADAM):
            st, msg, _ = _create(meta, None, kind, [bad])
            assert st == inval and ("eta" in msg or "non-finite" in msg), (bad, kind, msg)
    st, msg, _ = _create(meta, None, _lib.OPTIM_SGD, [0.1, 0.9])
    assert st == inval and "at most 1" in msg
    st, msg, _ = _create(meta, None, _lib.OPTIM_ADAM, [0.1, 0.99, 0.9, 1e-7, 0.0])
    assert st == inval and "at most 4" in msg
    # all arguments good but the model has no context: the reason is the host-only model, not the table
    for kind, hp in ((_lib.OPTIM_SGD, [0.1]), (_lib.OPTIM_MOMENTUM, [0.1, 0.8]), (_lib.OPTIM_ADAGRAD, [0.1]),
                     (_lib.OPTIM_ADAM, [0.0, 0.99, 0.9, 1e-7])):
        st, msg, h = _create(meta, None, kind, hp)
        assert st == inval and "host-only model" in msg and not h.value
    assert _lib.lib.rmx_optim_steps(None) == -1
    assert _lib.lib.rmx_optim_destroy(None) == _lib.RMX_OK
    assert _lib.lib.rmx_optim_apply(None, 1, None, None, None, None, None, None) == inval
    assert _lib.lib.rmx_train_step_ids(meta, None, None, 1, None, None, None, None) == inval


def test_get_bias_and_get_mats_on_a_host_only_model():
    m = rmx.DeepFM(2000, 39, 16, [24, 8])
    b = ctypes.c_float(-1.0)
    assert _lib.lib.rmx_model_get_bias(m._meta, ctypes.byref(b)) == _lib.RMX_E_INVALID  # never set
    assert _lib.lib.rmx_model_set_bias(m._meta, 0.25) == _lib.RMX_OK
    assert _lib.lib.rmx_model_get_bias(m._meta, ctypes.byref(b)) == _lib.RMX_OK and b.value == 0.25
    assert _lib.lib.rmx_model_get_bias(None, ctypes.byref(b)) == _lib.RMX_E_INVALID
    buf = np.zeros(m.matsLength(), np.float32)
    st = _lib.lib.rmx_model_get_mats(m._meta, _lib.ptr(buf, ctypes.c_float), len(buf))
    assert st == _lib.RMX_E_INVALID and b"host-only model" in _lib.lib.rmx_last_error()


def test_python_optimizer_rejects_bad_kind_and_hyper_names():
    m = rmx.DeepFM(2000, 39, 16, [24, 8])
    with pytest.raises(rmx.IllegalArgumentError):
        rmx.Optimizer(m, None, "rmsprop", eta=0.1)
    with pytest.raises(TypeError):
        rmx.Optimizer(m, None, "sgd", eta=0.1, momentum=0.9)
    with pytest.raises(TypeError):
        rmx.Optimizer(m, None, "adam", gamma=0.9)


# ----------------------------------------------------- ctypes declarations vs header ----
NEW = ["rmx_optim_create", "rmx_optim_destroy", "rmx_optim_steps", "rmx_optim_state_ptrs", "rmx_optim_apply",
       "rmx_train_step_ids", "rmx_model_get_mats", "rmx_model_get_bias"]


def _ctype_of(decl):
    """C parameter / return declaration -> the class of ctypes type _lib.py must use."""
    decl = re.sub(r"\bconst\b", "", decl).strip()
    if "*" in decl:
        return "ptr"
    base = decl.split()[0]
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
            "float": ctypes.c_float}[base]


def _is(ct, want):
    if want == "ptr":
        return ct is ctypes.c_void_p or ct is ctypes.c_char_p or hasattr(ct, "_type_") and hasattr(ct, "contents")
    return ct is want


def test_lib_declarations_match_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rmx.h")).read(), flags=re.S)
    sigs = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    for name in NEW:
        m = re.search(r"^\s*([\w\s\*]+?)\b%s\s*\(([^)]*)\)\s*;" % name, src, flags=re.M)
        assert m, "%s is not declared in include/rmx.h" % name
        assert name in sigs, "%s is not declared in rmx/_lib.py" % name
        res, args = sigs[name]
        assert _is(res, _ctype_of(m.group(1))), (name, "return type")
        params = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        assert len(params) == len(args), (name, params, args)
        for i, (p, a) in enumerate(zip(params, args)):
            assert _is(a, _ctype_of(p)), (name, i, p, a)
        fn = getattr(_lib.lib, name)
        assert fn.argtypes == args and fn.restype is res
