"""CPU: the surface of the sparse (lazy) Adam mode -- the two C entry points are declared, listed and exported under the
unchanged ABI version, their host-side argument checks answer without a device, and FusedAdam's `sparse` switch,
environment default, counters and pickled state behave as documented (the kernels: tests/test_gpu_sparse_adam.py)."""
import ctypes
import os
import pickle
import re

import pytest
import torch

import synthetic_scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gsr_sparse_step_workspace_bytes", "gsr_preprocess_backward_adam_raw_batched_sparse")
GSR_EINVAL, GSR_ENOSPACE = -1, -2


@pytest.fixture(autouse=True)
def _no_sink_left_behind():
    import diff_gaussian_rasterization as dgr

    yield
    dgr.set_deferred_backward_sink(None)


def test_symbols_are_declared_listed_and_exported_under_abi_15():
    from diff_gaussian_rasterization import _lib

    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in include/gsraster.h"
        assert n in _lib.SIGNATURES and hasattr(raw, n)
    assert _lib.ABI_VERSION == 15 and _lib.lib.gsr_abi_version() == 15
    # the header states the semantics and that the entry has no reference call site
    doc = src[src.index("Sparse Adam"):src.index("size_t gsr_sparse_step_workspace_bytes")]
    for phrase in ("radii[k,i] > 0", "-0.0 counts as zero", "A NaN counts as non-zero", "no reference call site"):
        assert phrase in doc, phrase
    # the declared parameter list and the ctypes table have the same length
    decl = code[code.index("gsr_preprocess_backward_adam_raw_batched_sparse("):]
    decl = decl[:decl.index(";")]
    assert decl.count(",") + 1 == len(_lib.SIGNATURES[NEW[1]][1]) == 36


def test_workspace_bytes_is_positive_and_monotone():
    from diff_gaussian_rasterization import _lib

    f = _lib.lib.gsr_sparse_step_workspace_bytes
    assert f(1) > 0 and f(0) > 0
    prev = 0
    for P in (1, 2, 3, 63, 64, 1000, 1001, 1_000_000, 6_000_000, 40_000_000, 2**31 - 1):
        n = f(P)
        assert n >= prev and n >= 4 * P and n % 8 == 0, (P, n)
        prev = n


def _args(**kw):
    """a well-formed argument list whose device pointers are made-up addresses: the checks must not dereference them"""
    VP, D6, I64 = ctypes.c_void_p * 6, ctypes.c_double * 6, ctypes.c_int64 * 6
    dev = lambda k: 0x7000_0000 + 0x10000 * k  # 16-byte aligned, never touched
    a = dict(P=1000, B=2, deg=3, M=16, xyz=dev(1), scaling=dev(2), smod=1.0, rotation=dev(3), f_dc=dev(4), f_rest=dev(5),
             opacity=dev(6), cams=dev(7), W=320, H=208, radii=dev(8), cov3D=dev(9), clamped=dev(10), g2=dev(11),
             gco=dev(12), grgb=dev(13), gstride=9, m=VP(*[dev(20 + t) for t in range(6)]),
             v=VP(*[dev(30 + t) for t in range(6)]), lrs=D6(*[1e-3] * 6), b1=D6(*[0.9] * 6), b2=D6(*[0.999] * 6),
             eps=D6(*[1e-15] * 6), steps=I64(*[2] * 6), grad_scale=1.0, dyn=None, skip=None, ws=dev(40), ws_bytes=None,
             active_out=None, num_active=None, stream=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        from diff_gaussian_rasterization import _lib

        a["ws_bytes"] = _lib.lib.gsr_sparse_step_workspace_bytes(max(a["P"], 0))
    return list(a.values())


def test_validation_codes_are_returned_without_a_device():
    from diff_gaussian_rasterization import _lib

    f = _lib.lib.gsr_preprocess_backward_adam_raw_batched_sparse
    for name in ("xyz", "scaling", "rotation", "f_dc", "f_rest", "opacity", "cams", "radii", "cov3D", "clamped", "g2",
                 "gco", "grgb", "m", "v", "b1", "b2", "eps", "lrs", "steps", "ws"):
        assert f(*_args(**{name: None})) == GSR_EINVAL, name
    VP = ctypes.c_void_p * 6
    assert f(*_args(m=VP(0x1000, 0x2000, None, 0x4000, 0x5000, 0x6000))) == GSR_EINVAL  # a null moment in the table
    assert f(*_args(M=4)) == GSR_EINVAL and f(*_args(M=15)) == GSR_EINVAL and f(*_args(M=17)) == GSR_EINVAL
    assert f(*_args(P=-1)) == GSR_EINVAL and f(*_args(B=0)) == GSR_EINVAL and f(*_args(W=-320)) == GSR_EINVAL
    assert f(*_args(gstride=-9)) == GSR_EINVAL and f(*_args(deg=4)) == GSR_EINVAL
    need = _lib.lib.gsr_sparse_step_workspace_bytes(1000)
    assert f(*_args(ws_bytes=need - 1)) == GSR_ENOSPACE and f(*_args(ws_bytes=0)) == GSR_ENOSPACE
    assert f(*_args(ws=0x7100_0004, ws_bytes=need + 64)) == GSR_ENOSPACE  # not 8-byte aligned
    assert f(*_args(P=0)) == 0
    assert f(*_args(P=0, xyz=None, ws=None, ws_bytes=0)) == 0


def _model():
    return S.SyntheticGaussianModel(64, 64, 48, seed=1)


def test_sparse_needs_fuse_backward():
    from fused_optim import FusedAdam

    m = _model()
    with pytest.raises(ValueError):
        FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, sparse=True)
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15)
    with pytest.raises(ValueError):
        opt.set_sparse(True)
    opt.set_fuse_backward(True)
    opt.set_sparse(True)
    assert opt.sparse is True
    opt.set_sparse(False)
    assert opt.sparse is False
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=True)
    assert opt.sparse and opt.sparse_steps == 0 and opt.dense_fallback_steps == 0 and opt.last_num_active is None


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_environment_default_is_read_at_construction(monkeypatch, value, on):
    from fused_optim import FusedAdam

    if value is None:
        monkeypatch.delenv("GSR_SPARSE_ADAM", raising=False)
    else:
        monkeypatch.setenv("GSR_SPARSE_ADAM", value)
    m = _model()
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True)
    assert opt.sparse is on
    assert FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=False).sparse is False
    assert FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=True).sparse is True
    # an optimizer that does not fuse the backward is never switched by the environment (and does not raise)
    assert FusedAdam(m.param_groups(), lr=0.0, eps=1e-15).sparse is False
    monkeypatch.setenv("GSR_SPARSE_ADAM", "0" if on else "1")  # read at construction, not later
    assert opt.sparse is on


def test_sparse_step_asks_the_pending_backward_for_the_sparse_launch():
    from fused_optim import FusedAdam

    calls = []

    class Pending:
        def __init__(self, params):
            self.params, self.versions = params, tuple(t._version for t in params)

        def fused_step(self, exp_avgs, exp_avg_sqs, lrs, b1, b2, eps, steps, grad_scale, cache=None, sparse=False):
            calls.append(sparse)

    m = _model()
    params = tuple(getattr(m, n) for n in ("_xyz", "_scaling", "_rotation", "_features_dc", "_features_rest", "_opacity"))
    opt = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=True)
    opt.offer(Pending(params))
    opt.step()
    opt.set_sparse(False)
    opt.offer(Pending(params))
    opt.step()
    assert calls == [True, False] and opt.sparse_steps == 1 and opt.fused_steps == 2 and opt.dense_fallback_steps == 0
    assert all(float(opt.state[p]["step"]) == 2 for p in params)  # the counters of all six groups advance every step


def test_state_dict_keys_are_unchanged_and_pickle_restores_defaults():
    from fused_optim import FusedAdam

    m = _model()
    plain = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=False)
    sparse = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=True)
    a, b = plain.state_dict(), sparse.state_dict()
    assert sorted(a) == sorted(b) == ["param_groups", "state"]
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert not any("sparse" in k for g in b["param_groups"] for k in g)
    back = pickle.loads(pickle.dumps(sparse))
    # (an optimizer pickles its defaults, state and param groups only) disarmed, as every unpickled optimizer: the mode
    # needs fuse_backward, so it comes back off with its counters at their defaults
    assert back.sparse is False and back.sparse_steps == 0 and back.dense_fallback_steps == 0
    assert back.fuse_backward is False and back.last_num_active is None
    assert sorted(back.state_dict()) == ["param_groups", "state"]
    # a state from before the mode existed: the new attributes get their defaults
    old = FusedAdam.__new__(FusedAdam)
    old.__setstate__({"defaults": plain.defaults, "state": {}, "param_groups": plain.param_groups})
    assert old.sparse is False and old.sparse_steps == 0 and old.dense_fallback_steps == 0
    assert old.last_num_active is None
