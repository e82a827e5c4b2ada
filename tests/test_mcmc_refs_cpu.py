"""CPU: the restatements of tests/mcmc_refs.py against known answers and identities, the C-ABI surface of csrc/mcmc.hip
(symbols, argument validation before any launch), RowArena.extend on host tensors and the fuse_backward restriction of
MCMCStrategy.add_regulariser_grads."""
import ctypes
import os
import re
from decimal import Decimal

import numpy as np
import pytest
import torch

import mcmc_refs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gsr_mcmc_noise", "gsr_mcmc_normals", "gsr_mcmc_reg_grad", "gsr_mcmc_relocate_apply",
               "gsr_mcmc_relocate_bytes", "gsr_mcmc_relocate_plan"]


# ------------------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in M.philox4x32_10(counter, key)) == want


def test_philox_rows_is_the_scalar_function():
    rows = np.array([0, 1, 77, 2 ** 31 - 1, 2 ** 32 + 5], dtype=np.uint64)
    seed = 0x299f31d0a4093822
    x = M.philox_rows(rows, 13, M.DOMAIN_NOISE, seed)
    for j, r in enumerate(rows):
        r = int(r)
        want = M.philox4x32_10((r & M.M32, r >> 32, 13, M.DOMAIN_NOISE), (seed & M.M32, seed >> 32))
        assert tuple(int(v) for v in x[:, j]) == want
    assert not np.array_equal(x, M.philox_rows(rows, 13, M.DOMAIN_RELOCATE, seed))  # the domains are separate streams


def test_the_device_source_states_the_same_philox_constants_and_domains():
    src = open(os.path.join(ROOT, "grendel-gs_amd", "csrc", "mcmc.hip")).read()
    for needle in ("0xD2511F53u", "0xCD9E8D57u", "0x9E3779B9u", "0xBB67AE85u", "DOMAIN_RELOCATE = 1u", "DOMAIN_NOISE = 2u",
                   "#pragma clang fp contract(off)"):
        assert needle in src, needle


# ------------------------------------------------------------------------------------------------------- relocation
@pytest.mark.parametrize("o", [0.0051, 0.5, 0.99])
def test_double_sum_is_the_hockey_stick_single_sum(o):
    """sum_{i=1..n} C(i-1,k) = C(n,k+1): the paper's double sum (image preservation for n Gaussians on one spot) is the
    single sum the kernel evaluates -- for every n the kernel accepts.  60-digit arithmetic: equal to 1e-50 relative."""
    for n in range(1, 52):
        o_new = M.relocation(o, n, 0.005)["o_raw"]
        a, b = M.double_sum_D(o_new, n), M.single_sum_D(o_new, n)
        assert a > 0 and abs(a - b) <= a * Decimal(10) ** -50, (o, n)


@pytest.mark.parametrize("o", [0.0051, 0.5, 0.99])
def test_one_gaussian_is_left_alone(o):
    r = M.relocation(o, 1, 0.005)
    o32 = float(np.float32(o))
    assert r["o_raw"] == o32 and r["f"] == 1.0 and abs(r["log_f"]) < 1e-50 and r["D"] == o32


def test_relocated_opacity_composes_back():
    """n Gaussians of opacity o' composite to 1 - (1 - o')^n = o"""
    for o in (0.0051, 0.5, 0.99):
        for n in (2, 7, 51):
            r = M.relocation(o, n, 0.0)
            assert abs(1 - (1 - r["o_raw"]) ** n - float(np.float32(o))) < 1e-14
            assert 0 < r["f"] <= 1.0  # the copies shrink


def test_sampling_frequencies_and_zero_weight():
    """10^5 draws over four weights (and a zero-weight row among them): each frequency within 5 sigma of w / sum(w)"""
    opacity = np.array([0.4, 0.004, 0.1, 0.25, 0.25], dtype=np.float32)  # row 1 is dead: weight 0
    w, dead = M.weights(opacity, 0.005)
    assert dead.tolist() == [False, True, False, False, False] and w[1] == 0
    assert w.tolist() == [int(np.float32(v) * 2 ** 24) if i != 1 else 0 for i, v in enumerate(opacity)]
    prefix = np.concatenate([[0], np.cumsum(w)])[:5].astype(np.uint64)
    total, n = int(w.sum()), 100_000
    x = M.philox_rows(np.arange(n), 3, M.DOMAIN_RELOCATE, 1234)
    hits = np.bincount([M.draw(prefix, total, a, b) for a, b in zip(x[0], x[1])], minlength=5)
    assert hits[1] == 0 and hits.sum() == n
    for i in (0, 2, 3, 4):
        p = int(w[i]) / total
        assert abs(hits[i] - n * p) <= 5 * (n * p * (1 - p)) ** 0.5, (i, hits[i], n * p)


def test_draw_picks_the_unique_row_and_plan_counts_add_up():
    w = np.array([5, 0, 0, 3, 0], dtype=np.uint64)
    prefix = np.array([0, 5, 5, 5, 8], dtype=np.uint64)
    for r, want in ((0, 0), (4, 0), (5, 3), (7, 3)):
        x = -(-(r << 64) // 8)  # the smallest x with (x * 8) >> 64 == r
        assert M.draw(prefix, 8, x & M.M32, x >> 32) == want
    rng = np.random.default_rng(0)
    opacity = (0.01 + 0.98 * rng.random(300)).astype(np.float32)
    opacity[::7] = 0.001
    src, count, (n_dead, n_alive) = M.relocate_plan(opacity, 9, 0.005, 42, 1)
    assert n_dead == 43 and n_alive == 257 and (src >= 0).sum() == n_dead + 9 == count.sum()
    assert np.all(src[:300][opacity > 0.005] == -1) and np.all(opacity[src[src >= 0]] > 0.005)
    assert np.array_equal(np.bincount(src[src >= 0], minlength=300), count)
    src0, _, _ = M.relocate_plan(np.full(4, 0.001, np.float32), 2, 0.005, 42, 1)
    assert src0.tolist() == [-1] * 6  # no live row: nothing is drawn


# ------------------------------------------------------------------------------------------------------------ C-ABI
def test_header_table_and_library_agree_on_the_new_symbols():
    from diff_gaussian_rasterization import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsraster.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(gsr_mcmc_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == NEW_SYMBOLS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES and hasattr(raw, n), n
    assert _lib.lib.gsr_abi_version() == 15  # additive entry points: the ABI stays
    import diff_gaussian_rasterization as dgr

    for n in ("mcmc_relocate_plan", "mcmc_relocate_apply", "mcmc_noise", "mcmc_normals", "mcmc_reg_grad"):
        assert callable(getattr(dgr, n))
    assert "mcmc" in __import__("importlib").import_module("csrc.build").UNITS


def test_entry_points_validate_before_any_launch():
    """dummy non-zero integers stand for device pointers: every call is refused, or returns, before anything is
    dereferenced or launched (this machine has no device)"""
    from diff_gaussian_rasterization._lib import lib

    d, EINVAL = 0x1000, -1
    need = lib.gsr_mcmc_relocate_bytes(1000)
    assert need >= 8 * 1000 and lib.gsr_mcmc_relocate_bytes(5000) > need and lib.gsr_mcmc_relocate_bytes(-1) == 0
    plan = lib.gsr_mcmc_relocate_plan
    assert plan(-1, 0, d, 0.005, 1, 0, d, d, d, d, 1 << 30, None) == EINVAL
    assert plan(10, -1, d, 0.005, 1, 0, d, d, d, d, 1 << 30, None) == EINVAL
    assert plan(2 ** 31 - 1, 1, d, 0.005, 1, 0, d, d, d, d, 1 << 40, None) == EINVAL  # src[] is int32
    for k in range(5):  # opacity, src, count, totals, workspace
        p = [d] * 5
        p[k] = None
        assert plan(1000, 3, p[0], 0.005, 1, 0, p[1], p[2], p[3], p[4], 1 << 30, None) == EINVAL, k
    assert plan(1000, 3, d, 0.005, 1, 0, d, d, d, d, need - 1, None) == EINVAL  # workspace too small
    assert plan(0, 3, None, 0.005, 1, 0, None, None, None, None, 0, None) == 0
    apply_ = lib.gsr_mcmc_relocate_apply
    one = (ctypes.c_void_p * 1)(d)
    w1, s1, r1 = (ctypes.c_int32 * 1)(1), (ctypes.c_int64 * 1)(1), (ctypes.c_int32 * 1)(2)
    assert apply_(-1, 0, d, d, d, 0.005, 51, 1, one, w1, s1, r1, None) == EINVAL
    for n_max in (0, 52, -3):
        assert apply_(10, 0, d, d, d, 0.005, n_max, 1, one, w1, s1, r1, None) == EINVAL
    for k in range(3):  # src, count, opacity
        p = [d] * 3
        p[k] = None
        assert apply_(10, 0, p[0], p[1], p[2], 0.005, 51, 1, one, w1, s1, r1, None) == EINVAL
    assert apply_(10, 0, d, d, d, 0.005, 51, 1, None, w1, s1, r1, None) == EINVAL
    assert apply_(10, 0, d, d, d, 0.005, 51, 33, one, w1, s1, r1, None) == EINVAL
    assert apply_(10, 0, d, d, d, 0.005, 51, 1, one, w1, s1, (ctypes.c_int32 * 1)(7), None) == EINVAL  # no such role
    assert apply_(10, 0, d, d, d, 0.005, 51, 1, one, (ctypes.c_int32 * 1)(3), s1, r1, None) == EINVAL  # OPACITY: width 1
    assert apply_(10, 0, d, d, d, 0.005, 51, 1, (ctypes.c_void_p * 1)(None), w1, s1, r1, None) == EINVAL
    assert apply_(0, 0, None, None, None, 0.005, 51, 1, one, w1, s1, r1, None) == 0
    noise = lib.gsr_mcmc_noise
    assert noise(-1, d, d, d, d, 1.0, None, 1, 0, None) == EINVAL
    for k in range(4):  # xyz, scaling, rotation, opacity (xi may be NULL)
        p = [d] * 4
        p[k] = None
        assert noise(10, p[0], p[1], p[2], p[3], 1.0, None, 1, 0, None) == EINVAL
    assert noise(10, d, d, d + 4, d, 1.0, None, 1, 0, None) == EINVAL  # the quaternion load is 16 bytes wide
    assert noise(0, None, None, None, None, 1.0, None, 1, 0, None) == 0
    assert lib.gsr_mcmc_normals(-1, 1, 0, d, None) == EINVAL and lib.gsr_mcmc_normals(10, 1, 0, None, None) == EINVAL
    assert lib.gsr_mcmc_normals(0, 1, 0, None, None) == 0
    reg = lib.gsr_mcmc_reg_grad
    assert reg(-1, d, d, 1.0, 1.0, d, d, None) == EINVAL
    for k in range(4):
        p = [d] * 4
        p[k] = None
        assert reg(10, p[0], p[1], 1.0, 1.0, p[2], p[3], None) == EINVAL
    assert reg(0, None, None, 1.0, 1.0, None, None, None) == 0


def test_wrappers_refuse_host_tensors():
    import diff_gaussian_rasterization as dgr

    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.mcmc_relocate_plan(torch.rand(8), 0, 0.005, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.mcmc_relocate_apply(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), torch.rand(8), 0.005,
                                [torch.zeros(8, 1)], [dgr.MCMC_ROLE_OPACITY])
    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.mcmc_noise(torch.zeros(8, 3), torch.zeros(8, 3), torch.ones(8, 4), torch.zeros(8, 1), 1.0)
    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.mcmc_normals(8, 0, 0, out=torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU"):
        dgr.mcmc_reg_grad(torch.zeros(8, 1), torch.zeros(8, 3), 1.0, 1.0, torch.zeros(8, 1), torch.zeros(8, 3))


# -------------------------------------------------------------------------------------------------------- host logic
def test_row_arena_extend_keeps_the_storage_and_copies_once():
    from row_arena import RowArena

    arena = RowArena(100, "cpu", capacity=130)
    t = torch.arange(300.0).reshape(100, 3)
    a = arena.extend("xyz", t, 105)
    assert a.shape == (105, 3) and torch.equal(a[:100], t) and a.data_ptr() != t.data_ptr()  # THE copy
    a[100:] = 7.0
    b = arena.extend("xyz", a, 130)
    assert b.shape == (130, 3) and b.data_ptr() == a.data_ptr() and torch.equal(b[:105], a)  # a longer view, no copy
    assert b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
    c = arena.extend("xyz", b, 130)
    assert c.data_ptr() == b.data_ptr() and arena.growths == 0 and arena.capacity == 130
    other = arena.extend("opacity", torch.zeros(100, 1), 130)
    assert other.data_ptr() != b.data_ptr() and arena.half_of("xyz", b) is not None
    # the halves of the event path are untouched by it: a destination is still the OTHER half
    dst = arena.destination("xyz", b, 130)
    assert dst.data_ptr() != b.data_ptr()


def test_strategy_arithmetic_and_the_fuse_backward_restriction():
    import synthetic_scene as S
    from fused_optim import FusedAdam
    from mcmc import MCMCStrategy, _mix_rank, install

    st = MCMCStrategy(cap_max=4300)
    assert [st.rows_after(p) for p in (4000, 4200, 4300, 5000)] == [4200, 4300, 4300, 5000]
    assert (st.min_opacity, st.noise_lr, st.opacity_reg, st.scale_reg, st.grow_factor, st.n_max) == \
        (0.005, 5e5, 0.01, 0.01, 1.05, 51)
    seeds = {_mix_rank(s, r) for s in (0, 1) for r in range(8)}
    assert len(seeds) == 16 and all(0 <= s < 2 ** 64 for s in seeds)  # the rank is mixed into the seed
    assert MCMCStrategy(10, rank=3).device_seed() == _mix_rank(0, 3) != MCMCStrategy(10, rank=0).device_seed()
    with pytest.raises(ValueError):
        MCMCStrategy(cap_max=10, n_max=52)
    m = S.SyntheticGaussianModel(64, 64, 48, seed=1)
    m.optimizer = FusedAdam(m.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True)
    with pytest.raises(ValueError, match="fuse_backward"):
        st.add_regulariser_grads(m)

    class Model:
        pass

    install(Model)
    assert all(callable(getattr(Model, n)) for n in ("mcmc_relocate_and_grow", "mcmc_inject_noise",
                                                     "mcmc_add_regulariser_grads"))


def test_noise_reference_gate_and_bound():
    """the restated update at the gate's two ends: a solid Gaussian stays, a faint one moves along Sigma xi; the bound is
    positive and dominated by the final add where nothing moves"""
    xyz = np.array([[1.0, 2.0, 3.0]] * 2)
    s = np.log(np.array([[0.1, 0.2, 0.3]] * 2))
    q = np.array([[2.0, 0, 0, 0]] * 2)  # identity rotation, un-normalised
    op = np.array([5.0, -20.0])  # opacity 0.993 and 2e-9
    xi = np.array([[1.0, -1.0, 0.5]] * 2)
    out, bound, disp = M.noise(xyz, s, q, op, 2.0, xi)
    assert np.all(np.abs(disp[0]) < 1e-40) and np.allclose(bound[0], M.U * np.abs(xyz[0]), rtol=1e-6)
    g = 1 / (1 + np.exp(-100 * (1 / (1 + np.exp(-20.0)) - 0.995)))
    assert np.allclose(out[1] - xyz[1], 2.0 * g * np.array([0.01, -0.04, 0.045]), rtol=1e-12)
    assert np.all(bound > 0)
    go, gs = M.reg_grads(np.array([0.0]), np.array([[0.0, 1.0, -1.0]]), 2.0, 3.0)
    assert np.allclose(go, 0.5) and np.allclose(gs, 3.0 * np.exp([0.0, 1.0, -1.0]))
