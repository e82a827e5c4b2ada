"""Staging of the loss masks next to the ground-truth bands (gaussian_renderer/loss_distribution.py, set_loss_masks): a
three-rank gloo run on the CPU, with local and with rank-0-only storage.  Every rank ends up with exactly the mask rows
of the bands it renders -- for [H, W] and for [1, H, W] masks, for batches in which only some cameras carry one -- the
ground-truth bands are still right, and with the switch off nothing is staged."""
import multiprocessing as mp
import os
import socket
import sys
import traceback

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _mask_image(W, H, seed):
    g = torch.Generator().manual_seed(900 + seed)
    return torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8)


def _mask_worker(rank, world, port, q):
    try:
        for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
            if p not in sys.path:
                sys.path.insert(0, p)
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
        torch.set_num_threads(1)
        import synthetic_scene as S
        import utils.general_utils as utils
        from gaussian_renderer import loss_distribution as LD
        from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

        utils.init_distributed(backend="gloo")
        W, H, bsz = 160, 112, 2
        utils.set_img_size(H, W)
        assert LD.get_loss_masks() is False  # off by default
        seen_rows = 0
        # which cameras carry a mask, and in which of the two accepted shapes
        layouts = [("2d", None), ("3d", "2d"), (None, "3d")]
        for storage in (False, True):
            for on in (True, False):
                for layout in layouts:
                    LD.set_loss_masks(on)
                    utils.set_args(utils.default_args(bsz=bsz, distributed_dataset_storage=storage))
                    cams = S.orbit_cameras(bsz, W, H)
                    full = [S.make_gt_image(W, H, seed=40 + k) for k in range(bsz)]
                    masks = [_mask_image(W, H, k) for k in range(bsz)]
                    for k, c in enumerate(cams):
                        holder = not storage or rank == 0
                        # distributed storage: only the first rank of the node holds the pixels; the others know which
                        # cameras carry a mask (has_alpha_mask), not what is in it
                        c.original_image_backup = full[k] if holder else None
                        shaped = None if layout[k] is None else (masks[k] if layout[k] == "2d" else masks[k][None])
                        c.alpha_mask_backup = shaped if holder else None
                        if storage:
                            c.has_alpha_mask = layout[k] is not None
                        assert LD.camera_carries_mask(c) == (layout[k] is not None)
                    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
                    strategies, tasks = start_strategy_final(cams, hist)
                    LD.load_camera_from_cpu_to_all_gpu(cams, strategies, tasks)
                    for (k, l, r) in tasks[rank]:
                        y0, y1 = l * 16, min(r * 16, H)
                        what = (storage, on, layout, k, l, r)
                        assert torch.equal(cams[k].original_image, full[k][:, y0:y1, :]), what
                        got = getattr(cams[k], "alpha_mask", None)
                        if on and layout[k] is not None:
                            assert got is not None and got.dtype == torch.uint8, what
                            assert tuple(got.shape) == (1, y1 - y0, W) and got.is_contiguous(), what
                            assert torch.equal(got[0], masks[k][y0:y1]), what
                            seen_rows += y1 - y0
                        else:
                            assert got is None, what
        LD.set_loss_masks(False)
        # the run did stage masks somewhere: every rank renders a band of a masked camera in at least one layout
        total = torch.tensor([seen_rows])
        dist.all_reduce(total)
        assert int(total) > 0 and seen_rows > 0, (rank, seen_rows)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc()))


def test_mask_band_staging_local_and_distributed_storage():
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mask_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in results:
        assert msg == "ok", f"rank {rank}:\n{msg}"


def test_switch_and_environment_default():
    """set_loss_masks / get_loss_masks, and GSR_LOSS_MASKS=1 as the default of a fresh interpreter"""
    import subprocess

    for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    from gaussian_renderer import loss_distribution as LD

    was = LD.get_loss_masks()
    try:
        LD.set_loss_masks(True)
        assert LD.get_loss_masks() is True
        LD.set_loss_masks(0)
        assert LD.get_loss_masks() is False
    finally:
        LD.set_loss_masks(was)
    code = ("import sys; sys.path[:0] = [%r, %r]; from gaussian_renderer import loss_distribution as LD; "
            "print(LD.get_loss_masks())" % (os.path.join(ROOT, "grendel-gs_amd"), ROOT))
    for value, want in (("1", "True"),):  # (unset: the three-rank run above asserts the default is off)
        env = dict(os.environ)
        env.pop("GSR_LOSS_MASKS", None)
        if value is not None:
            env["GSR_LOSS_MASKS"] = value
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == want, (value, out)
