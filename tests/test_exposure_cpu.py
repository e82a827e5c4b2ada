"""Host side of the per-camera exposure compensation (grendel-gs_amd/exposure.py; include/gsraster.h, N1x): the model's
initial value, checkpoint round trip and learning-rate schedule, the gradient all-reduce on a two-rank gloo group, the
torch helper, and the new C-ABI names (header, ctypes table, library)."""
import ctypes
import os
import re
import socket
import sys
import traceback

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gsr_l1_ssim_forward_exposure", "gsr_l1_ssim_exposure_num_partials", "gsr_l1_ssim_backward_exposure"]


def _model(n=5, **kw):
    from exposure import ExposureModel

    return ExposureModel(n, device="cpu", **kw)


def test_model_initialises_to_identity():
    m = _model(5)
    want = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
    assert m.exposure.shape == (5, 3, 4) and m.exposure.dtype == torch.float32 and m.exposure.requires_grad
    for k in range(5):
        assert torch.equal(m.exposure[k].detach(), want)
    cam = type("Cam", (), {"uid": 3})()
    row = m.of(cam)
    assert torch.equal(row.detach(), want)
    row.sum().backward()  # a differentiable view: only row 3 of the parameter receives a gradient
    g = m.exposure.grad
    assert bool((g[3] == 1).all()) and float(g.abs().sum()) == 12.0
    assert bool((m.exp_avg == 0).all()) and bool((m.exp_avg_sq == 0).all()) and m.steps == 0


def test_state_dict_round_trip_is_exact():
    gen = torch.Generator().manual_seed(5)
    a = _model(4)
    with torch.no_grad():
        a.exposure.add_(0.1 * torch.randn(4, 3, 4, generator=gen))
        a.exp_avg.copy_(torch.randn(4, 3, 4, generator=gen))
        a.exp_avg_sq.copy_(torch.rand(4, 3, 4, generator=gen))
    a.steps = 17
    state = a.state_dict()
    with torch.no_grad():
        a.exposure.zero_()  # the state is a copy, not a view of the live tensors
    b = _model(4)
    b.load_state_dict(state)
    for name in ("exposure", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(b, name).detach(), state[name]), name
    assert b.steps == 17 and b.exposure.grad is None and b.exposure.requires_grad
    assert bool((state["exposure"] != 0).any())
    try:
        _model(3).load_state_dict(state)
    except ValueError:
        pass
    else:
        raise AssertionError("a state of another camera count must be refused")


def test_learning_rate_schedule():
    m = _model(2, lr_init=0.01, lr_final=0.001, max_steps=30000)
    assert m.lr_at(0) == 0.01
    assert abs(m.lr_at(30000) - 0.001) <= 1e-18 + 1e-15 * 0.001
    assert m.lr_at(10 ** 9) == m.lr_at(30000)  # held at its final value
    mid = m.lr_at(15000)
    assert abs(mid - (0.01 * 0.001) ** 0.5) <= 1e-12  # exponential decay: the geometric mean half-way
    vals = [m.lr_at(t) for t in range(0, 30001, 1000)]
    assert all(a > b for a, b in zip(vals, vals[1:]))
    ratios = [b / a for a, b in zip(vals, vals[1:])]
    assert max(ratios) - min(ratios) < 1e-12  # a constant factor per step


def test_step_has_no_cpu_path():
    m = _model(2)
    m.step()  # no gradient: nothing to do, nothing counted
    assert m.steps == 0
    m.exposure.grad = torch.ones_like(m.exposure)
    try:
        m.step()
    except RuntimeError as exc:
        assert "no CPU path" in str(exc)
    else:
        raise AssertionError("a host parameter must be refused")


def test_apply_exposure_matches_the_definition():
    from exposure import apply_exposure

    gen = torch.Generator().manual_seed(1)
    x = torch.rand(3, 5, 7, generator=gen, dtype=torch.float64)
    E = torch.randn(3, 4, generator=gen, dtype=torch.float64)
    want = torch.stack([E[c, 0] * x[0] + E[c, 1] * x[1] + E[c, 2] * x[2] + E[c, 3] for c in range(3)])
    assert torch.allclose(apply_exposure(x, E), want, rtol=1e-14, atol=1e-14)
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
    assert torch.equal(apply_exposure(x.float(), eye), x.float())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_grad(rank, n):
    return torch.arange(n * 12, dtype=torch.float32).reshape(n, 3, 4) * (rank + 1) + 0.25 * rank


def _sync_worker(rank, world, port, q):
    try:
        for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        torch.set_num_threads(1)
        import torch.distributed as dist
        import utils.general_utils as utils
        from exposure import ExposureModel

        utils.init_distributed(backend="gloo")
        n = 4
        m = ExposureModel(n, device="cpu")
        m.exposure.grad = _fake_grad(rank, n)
        m.sync_grads(utils.DEFAULT_GROUP)
        want = sum(_fake_grad(r, n) for r in range(world))
        assert torch.equal(m.exposure.grad, want), "not the exact sum"
        # a rank without a gradient (it rendered nothing) still takes part and receives the others' sum
        m.exposure.grad = None if rank == 1 else _fake_grad(rank, n)
        m.sync_grads(utils.DEFAULT_GROUP)
        assert torch.equal(m.exposure.grad, _fake_grad(0, n))
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def test_sync_grads_sums_over_a_two_rank_group():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in results:
        assert msg == "ok", f"rank {rank}:\n{msg}"


def test_sync_grads_without_a_group_is_a_no_op():
    m = _model(2)
    m.exposure.grad = _fake_grad(0, 2)
    m.sync_grads(None)
    assert torch.equal(m.exposure.grad, _fake_grad(0, 2))


def test_new_entry_points_are_declared_bound_and_exported():
    from diff_gaussian_rasterization import _lib

    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/gsraster.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype"
        assert hasattr(raw, name), f"{name} is not exported by the library"
    lib = _lib.lib
    assert lib.gsr_abi_version() == 15  # purely additive
    # pure host arithmetic: one 12-float row per 32x32 tile
    assert lib.gsr_l1_ssim_exposure_num_partials(1080, 1920) == 34 * 60
    assert lib.gsr_l1_ssim_exposure_num_partials(33, 37) == 4 and lib.gsr_l1_ssim_exposure_num_partials(0, 37) == 0
    # refused before any device work (dummy non-zero integers stand for device pointers)
    d = 0x1000
    for C in (1, 4):
        assert lib.gsr_l1_ssim_forward_exposure(C, 8, 8, d, 64, d, d, None, None, None, None, d, None) == -1
        assert lib.gsr_l1_ssim_backward_exposure(C, 8, 8, d, 64, d, d, d, d, d, d, 1.0, 1.0, d, 64, None, d, d, d,
                                                 None) == -1
    assert lib.gsr_l1_ssim_forward_exposure(3, 8, 8, d, 64, d, d, None, None, None, None, None, None) == -1
    assert lib.gsr_l1_ssim_forward_exposure(3, 8, 8, d, 64, d, None, None, None, None, None, d, None) == -1
    for null in (16, 17, 18):  # exposure, exposure_partials, grad_exposure
        a = [3, 8, 8, d, 64, d, d, d, d, d, d, 1.0, 1.0, d, 64, None, d, d, d, None]
        a[null] = None
        assert lib.gsr_l1_ssim_backward_exposure(*a) == -1


def test_loss_hook_defaults_to_none_and_the_operator_has_no_cpu_fallback():
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import loss_distribution as ld

    assert ld.get_exposure_model() is None
    m = _model(2)
    ld.set_exposure_model(m)
    try:
        assert ld.get_exposure_model() is m
    finally:
        ld.set_exposure_model(None)
    assert ld.get_exposure_model() is None
    try:
        dgr.fused_band_loss_exposure(torch.zeros(3, 4, 4), m.exposure[0], torch.zeros(3, 4, 4, dtype=torch.uint8), 0, 4,
                                     0.2, 48)
    except RuntimeError as exc:
        assert "no CPU fallback" in str(exc)
    else:
        raise AssertionError("host tensors must be refused")
