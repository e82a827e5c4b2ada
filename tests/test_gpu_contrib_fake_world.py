"""-m gpu: gaussian_renderer.score_contributions for W in {2, 4} ranks on ONE device over the asynchronous stand-in
collectives of tests/fake_world.py, against the same scene on one rank.

Every fake rank owns a contiguous shard of the scene, so the rows a band receives are in the single-rank order and the
lists are the single-rank lists restricted to the band: the owners' `scores`, concatenated, equal the W = 1 `scores` --
hits exactly, wmax bit for bit, wsum within the rounding of a row's fp64 additions (4 x tiles of them at most, per
camera).  A Gaussian that lies across two bands of one camera comes back to its owner twice: its hits are the sum of the
bands' (recomputed here band by band on one rank with the plain call), its wmax the larger.  Every rank takes part in
every camera's return trip -- at W = 4 with two cameras per batch half the ranks render no part of a camera -- and a
rank that leaves one out surfaces as CollectiveMismatch, not as a hang."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, WD, H = 4000, 192, 160          # 12 x 10 tiles: bands of at least two tile rows at W = 4
SCALE = 0.02
CAMS = 2


def _setup(utils, gr, wd, bsz):
    utils.set_args(utils.default_args(bsz=bsz, no_heuristics_update=True))
    utils.set_img_size(H, WD)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()


def _score(model, cams, hist, bsz, dev, skip_last=False):
    """-> (ContributionStats of the model's rows over all cameras, [(gpu_ids, division_pos)] per camera)"""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import score_contributions
    from gaussian_renderer.workload_division import start_strategy_final

    scores = dgr.ContributionStats(model._xyz.shape[0], dev)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    parts = []
    for b0 in range(0, len(cams), bsz):
        batch = cams[b0:b0 + bsz]
        strategies, _ = start_strategy_final(batch, hist)
        parts += [(list(s.gpu_ids), list(s.division_pos)) for s in strategies]
        if skip_last and b0 + bsz >= len(cams):
            batch, strategies = batch[:-1], strategies[:-1]
        assert score_contributions(batch, model, pipe, bg, strategies, scores) is scores
    return scores, parts


def _run_ranks(dev, world, bsz, skip_rank=None):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import synthetic_scene as S
    import utils.general_utils as utils
    from fake_world import FakeWorld
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal

    fw = FakeWorld(world, dev)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        _setup(utils, gr, wd, bsz)
        model = S.SyntheticGaussianModel(N, WD, H, seed=5, rank=rank, world_size=world, device=dev, scale_coef=SCALE)
        cams = S.orbit_cameras(CAMS, WD, H, device=dev)
        hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
        scores, parts = _score(model, cams, hist, bsz, dev, skip_last=(rank == skip_rank))
        return dict(hits=scores.hits.clone(), wmax=scores.wmax.clone(), wsum=scores.wsum.clone(), parts=parts)

    return fw.run(rank_main, timeout=120), fw


def _run_single(dev, bsz, parts):
    """the whole scene on one rank -> (scores, per camera and band: a ContributionStats of the band's tiles alone)"""
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import synthetic_scene as S
    import utils.general_utils as utils
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    _setup(utils, gr, wd, bsz)
    model = S.SyntheticGaussianModel(N, WD, H, seed=5, device=dev, scale_coef=SCALE)
    cams = S.orbit_cameras(CAMS, WD, H, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    scores, _ = _score(model, cams, hist, bsz, dev)
    # band by band with the plain call: the view's lists and K8's n_contrib once, then one mask per band
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    gx, gy = (WD + 15) // 16, (H + 15) // 16
    bands = []
    with torch.no_grad():
        for k, cam in enumerate(cams):
            strategies, _ = start_strategy_final([cam], hist)
            pkg = distributed_preprocess3dgs_and_all2all_final([cam], model, pipe, bg, batched_strategies=strategies,
                                                               mode="test")
            m2, co = pkg["batched_means2D_redistributed"][0], pkg["batched_conic_opacity_redistributed"][0]
            rgb, radii = pkg["batched_rgb_redistributed"][0], pkg["batched_radii_redistributed"][0]
            depths = pkg["batched_depths_redistributed"][0]
            full = torch.ones(gx * gy, dtype=torch.uint8, device=dev)
            _, _, _, nc = pkg["batched_rasterizers"][0].render_gaussians(m2, co, rgb, depths, radii, None, None, {})
            point_list, ranges, _ = dgr.bin_gaussians(m2.contiguous(), depths.contiguous(), radii.contiguous(),
                                                      co.contiguous(), full, WD, H)
            per_band = []
            div = parts[k][1]
            for j in range(len(div) - 1):
                mask = torch.zeros(gy, gx, dtype=torch.uint8, device=dev)
                mask[div[j]:div[j + 1]] = 1
                st = dgr.ContributionStats(N, dev)
                dgr.contribution_stats(ranges, point_list, m2, co, nc, mask.view(-1), WD, H, st)
                per_band.append(st)
            bands.append(per_band)
    torch.cuda.synchronize()
    return scores, bands


@pytest.mark.parametrize("world,bsz", [(2, 1), (4, 2)])
def test_owners_scores_equal_the_single_rank_scores(device, world, bsz):
    res, fw = _run_ranks(device, world, bsz)
    parts = res[0]["parts"]
    assert all(r["parts"] == parts for r in res), "the ranks disagree on the partition"
    assert all(len(div) >= 3 for _, div in parts), "every camera is cut into at least two bands"
    if world == 4:
        assert all(len(ids) < world for ids, _ in parts), "some rank renders no part of each camera"
    # per camera: the exchange and the return trip, on every rank (checked at every rendezvous)
    a2a = sum(1 for _, tag in fw.log if tag == "all_to_all_single")
    assert a2a == 2 * CAMS, fw.log
    ref, bands = _run_single(device, bsz, parts)
    hits = torch.cat([r["hits"] for r in res])
    wmax = torch.cat([r["wmax"] for r in res])
    wsum = torch.cat([r["wsum"] for r in res])
    assert hits.shape[0] == N and res[0]["hits"].shape[0] == (N + world - 1) // world
    assert int((ref.hits > 0).sum()) > N // 10, "the scene blends too little to show anything"
    assert torch.equal(hits, ref.hits)
    assert torch.equal(wmax.view(torch.int32), ref.wmax.view(torch.int32))
    n_add = CAMS * 4 * ((WD + 15) // 16) * ((H + 15) // 16)  # fp64 additions into one row, at most
    err = (wsum - ref.wsum).abs()
    print(f"CONTRIB-WORLD W={world}: rows with hits {int((hits > 0).sum())}, worst wsum deviation "
          f"{float((err / ref.wsum.clamp(min=1e-300)).max()):.3g} (bound {n_add * 2.0 ** -53:.3g})")
    assert bool((err <= n_add * 2.0 ** -53 * ref.wsum).all())
    # a Gaussian that lies across two bands of a camera: both bands' hits, the larger wmax
    across = torch.cat([torch.nonzero(torch.stack([st.hits > 0 for st in per_band]).sum(dim=0) >= 2).reshape(-1)
                        for per_band in bands])
    assert across.numel() > 0, "no Gaussian is blended in two bands of one camera"
    flat = [st for per_band in bands for st in per_band]
    tot_hits = sum(st.hits for st in flat)
    tot_wmax = torch.stack([st.wmax for st in flat]).amax(dim=0)
    assert torch.equal(hits[across], tot_hits[across]) and torch.equal(wmax[across], tot_wmax[across])
    assert torch.equal(hits, tot_hits) and torch.equal(wmax, tot_wmax)


def test_a_rank_that_skips_a_return_trip_is_a_mismatch_not_a_hang(device):
    from fake_world import CollectiveMismatch

    with pytest.raises(CollectiveMismatch):
        _run_ranks(device, 2, 1, skip_rank=1)
