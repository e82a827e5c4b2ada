"""-m gpu: the inverse-depth map through the Python layers -- gaussian_renderer.set_invdepth, render_final's
pkg["batched_invdepth"], loss_distribution.invdepth_l1 -- against the float64 oracle chain (O.preprocess, O.bin_and_sort,
O.render with rgb = (1 / depth, 0, 0), bg = 0; depth = ([p,1] @ view)[2] kept differentiable).

Scene: 2 000 Gaussians at 96 x 64, SH degree 1, one rank.  The prior is the oracle's own map plus an offset of at least
0.05 of either sign per pixel, so no pixel sits at the kink of the L1.  Map, loss and the gradients in xyz, opacity,
scaling and rotation meet the norm-wise 1e-4 bar of tests/test_gpu_parity.py; the xyz gradient with the depths detached
(in the oracle) is far from both, so the depth path is really connected.  With the switch off and on the colour image and
the colour-only gradients keep their bits.  The refusals raise: FusedAdam(fuse_backward=True) dense and sparse, graph
capture, gradients at world size 2.  Two bands on tests/fake_world.py: their maps SUM to the one-rank map bit for bit."""
import pytest
import torch

import synthetic_scene as S
from helpers import cam_kwargs, rel_err

pytestmark = pytest.mark.gpu

N, W, H, DEG, SCALE, SEED, VIEW = 2000, 96, 64, 1, 0.01, 5, 1
RTOL = 1e-4
NAMES = ["_xyz", "_opacity", "_scaling", "_rotation"]
ALL = NAMES + ["_features_dc", "_features_rest"]


def _single_rank(dev):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils

    utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = 0, 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    wd._BALANCE["mode"] = "exact"
    gr._PLANNERS.clear()


def _render(model, dev, invdepth, mode="train"):
    """-> (image [3,H,W], the map [1,H,W] or None, pkg) of view VIEW through the product's two calls"""
    import gaussian_renderer as gr
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    cams = S.orbit_cameras(4, W, H, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), 1, 0)
    strategies, _ = start_strategy_final([cams[VIEW]], hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    was = gr.get_invdepth()
    gr.set_invdepth(invdepth)
    try:
        pkg = distributed_preprocess3dgs_and_all2all_final([cams[VIEW]], model, pipe, bg, batched_strategies=strategies,
                                                           mode=mode)
        images, _ = render_final(pkg, strategies)
    finally:
        gr.set_invdepth(was)
    return images[0], (pkg["batched_invdepth"][0] if "batched_invdepth" in pkg else None), pkg


def _model(dev):
    return S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, device=dev, scale_coef=SCALE)


@pytest.fixture(scope="module")
def oracle():
    """the float64 chain on the host, once: map, prior, mask, loss, gradients with and without the depth path"""
    from oracle import torch_oracle as O

    m = _model("cpu")
    cam = S.orbit_cameras(4, W, H)[VIEW]
    kw = cam_kwargs(cam, DEG)
    mask = torch.ones((H + 15) // 16 * ((W + 15) // 16), dtype=torch.bool)
    raw = {n: getattr(m, n).detach().double().clone().requires_grad_(True) for n in ALL}

    def chain(detach_depth):
        xyz = raw["_xyz"]
        shs = torch.cat([raw["_features_dc"], raw["_features_rest"]], dim=1)
        m2, rgb, co, radii, depths = O.preprocess(xyz, torch.exp(raw["_scaling"]),
                                                  torch.nn.functional.normalize(raw["_rotation"]), shs,
                                                  torch.sigmoid(raw["_opacity"]), **kw)
        z = (torch.cat([xyz, torch.ones(N, 1, dtype=torch.float64)], dim=1) @ kw["viewmatrix"].double())[:, 2]
        seen = radii > 0
        v = torch.where(seen, 1.0 / torch.where(seen, z, torch.ones_like(z)), torch.zeros_like(z))
        if detach_depth:
            v = v.detach()
        binning = O.bin_and_sort(m2, radii, depths, mask, W, H)
        img, _, _ = O.render(m2, co, torch.stack([v, torch.zeros_like(v), torch.zeros_like(v)], dim=1), depths, radii,
                             mask, bg=torch.zeros(3, dtype=torch.float64), W=W, H=H, binning=binning)
        return img[0]

    inv = chain(False)
    gen = torch.Generator().manual_seed(9)
    off = (0.05 + 0.2 * torch.rand(H, W, generator=gen)) * torch.where(torch.rand(H, W, generator=gen) < 0.5, -1.0, 1.0)
    target = (inv.detach() + off).float()
    valid = (torch.rand(H, W, generator=gen) < 0.8).float()

    def loss_of(x):
        return ((x - target.double()).abs() * valid.double()).mean()

    loss = loss_of(inv)
    grads = dict(zip(NAMES, torch.autograd.grad(loss, [raw[n] for n in NAMES])))
    detached = torch.autograd.grad(loss_of(chain(True)), [raw["_xyz"]])[0]
    return dict(inv=inv.detach(), target=target, valid=valid, loss=float(loss), grads=grads, xyz_detached=detached)


def test_map_loss_and_gradients_against_the_float64_oracle(device, oracle):
    from gaussian_renderer.loss_distribution import invdepth_l1

    _single_rank(device)
    model = _model(device)
    image, inv, pkg = _render(model, device, True)
    assert inv is not None and inv.shape == (1, H, W) and image.shape == (3, H, W)
    loss = invdepth_l1(inv, oracle["target"].to(device)[None], oracle["valid"].to(device)[None], 0, H)
    loss.backward()
    torch.cuda.synchronize()
    e_map, e_loss = rel_err(inv[0], oracle["inv"]), abs(float(loss) - oracle["loss"]) / oracle["loss"]
    print(f"INVDEPTH-PIPE map rel err {e_map:.3g}, loss {float(loss):.9g} vs {oracle['loss']:.9g} ({e_loss:.3g})")
    assert float(oracle["inv"].max()) > 0.05 and e_map < RTOL and e_loss < RTOL
    for n in NAMES:
        e = rel_err(getattr(model, n).grad, oracle["grads"][n])
        print(f"INVDEPTH-PIPE d{n}: rel err {e:.3g}")
        assert e < RTOL, n
    # the depth path is connected: without it the xyz gradient is somewhere else entirely
    gap = rel_err(oracle["xyz_detached"], oracle["grads"]["_xyz"])
    print(f"INVDEPTH-PIPE d_xyz with the depths detached (oracle): {gap:.3g} away")
    assert gap > 100 * RTOL and rel_err(model._xyz.grad, oracle["xyz_detached"]) > 100 * RTOL
    # band rows: the loss of two half bands, each a mean over its rows, averages to the whole (equal heights)
    with torch.no_grad():
        t, v = oracle["target"].to(device)[None], oracle["valid"].to(device)[None]
        halves = 0.5 * (invdepth_l1(inv, t, v, 0, H // 2) + invdepth_l1(inv, t, v, H // 2, H))
    assert abs(float(halves) - float(loss)) <= 1e-6 * float(loss)


def test_switch_off_and_on_keep_the_colour_bits(device):
    _single_rank(device)
    wgt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).to(device)
    out = {}
    for on in (False, True):
        model = _model(device)
        image, inv, pkg = _render(model, device, on)
        assert (inv is not None) == on and ("batched_invdepth" in pkg) == on
        assert all(("invdepth" in ca) == on for ca in pkg["batched_cuda_args"])
        (image * wgt).sum().backward()
        torch.cuda.synchronize()
        out[on] = (image.detach().clone(), {n: getattr(model, n).grad.clone() for n in ALL})
    assert torch.equal(out[False][0], out[True][0]), "the colour image changed with the switch"
    for n in ALL:
        assert torch.equal(out[False][1][n], out[True][1][n]), f"the colour-only gradient of {n} changed with the switch"
    assert bool(out[True][1]["_xyz"].any())


@pytest.mark.parametrize("sparse", [False, True])
def test_fused_backward_refuses_the_maps_gradient(device, sparse):
    from fused_optim import FusedAdam

    _single_rank(device)
    model = _model(device)
    opt = FusedAdam(model.param_groups(), lr=0.0, eps=1e-15, fuse_backward=True, sparse=sparse)
    try:
        with pytest.raises(ValueError, match="fuse_backward=False"):
            _render(model, device, True)
        with torch.no_grad():  # forward only: nothing to refuse
            _, inv, _ = _render(model, device, True, mode="test")
        assert inv is not None and not inv.requires_grad
    finally:
        opt.set_fuse_backward(False)


def test_graph_capture_refuses_the_map(device, monkeypatch):
    import diff_gaussian_rasterization as dgr
    from helpers import settings_from

    g = S.make_gaussians(300, W, H, seed=3, scale_coef=0.02)
    cam = S.orbit_cameras(4, W, H)[0]
    rast = dgr.GaussianRasterizer(settings_from(cam, torch.zeros(3), sh_degree=DEG, device=device))
    with torch.no_grad():
        m2, rgb, co, radii, depths = rast.preprocess_gaussians(*[g[k].to(device) for k in
                                                                 ("means3D", "scales", "rotations", "shs", "opacities")], {})
        ca = {"invdepth": True}
        rast.render_gaussians(m2, co, rgb, depths, radii, None, None, ca)
        inv = rast.render_invdepth(m2, co, depths, ca)
        assert inv.shape == (H, W) and bool(inv.any())
        with pytest.raises(RuntimeError, match="cuda_args\\['invdepth'\\]"):
            rast.render_invdepth(m2, co, depths, {})
        monkeypatch.setattr(dgr, "_CAPTURE", [object()])  # what capturing() returns inside a graph capture
        with pytest.raises(RuntimeError, match="capture"):
            rast.render_gaussians(m2, co, rgb, depths, radii, None, None, {"invdepth": True})
        with pytest.raises(RuntimeError, match="capture"):
            rast.render_invdepth(m2, co, depths, ca)
        monkeypatch.undo()
    assert dgr.capturing() is None


def test_evaluation_returns_the_map_of_every_scored_camera(device):
    """training_report(invdepth=True): one [H,W] map per scored camera, bit-equal to the renderer's own map of that
    camera; the numbers of the report are those of the plain call, and the switch is back off afterwards"""
    import evaluation
    import gaussian_renderer as gr
    import utils.general_utils as utils

    class Scene:
        def __init__(self, gaussians, cams):
            self.gaussians, self._cams = gaussians, cams

        def getTrainCameras(self):
            return []

        def getTestCameras(self):
            return self._cams

    _single_rank(device)
    model = _model(device)
    cams = S.orbit_cameras(4, W, H, device=device)
    for k, c in enumerate(cams):
        c.uid = 100 + k
        c.original_image_backup = S.make_gt_image(W, H, seed=20 + k, device=device)
    bg = torch.tensor([0.1, 0.2, 0.3], device=device)
    pipe = type("P", (), {"debug": False})()
    plain = evaluation.training_report(1, [1], Scene(model, cams), pipe, bg)
    report = evaluation.training_report(1, [1], Scene(model, cams), pipe, bg, invdepth=True)
    assert not gr.get_invdepth() and "invdepth" not in plain["test"]
    maps = report["test"].pop("invdepth")
    # (the cameras of an epoch are drawn in a random order; the means over them do not depend on it beyond rounding)
    assert sorted(report["test"]["cameras"]) == sorted(plain["test"]["cameras"]) == [100, 101, 102, 103]
    for k in ("l1", "psnr"):
        assert abs(report["test"][k] - plain["test"][k]) <= 1e-12 * abs(plain["test"][k])
    assert report["test"]["num_cameras"] == plain["test"]["num_cameras"] == len(maps) == 4
    assert all(m.shape == (H, W) and bool(m.any()) for m in maps)
    _single_rank(device)
    with torch.no_grad():
        _, one, _ = _render(model, device, True, mode="test")
    at = report["test"]["cameras"].index(100 + VIEW)
    assert torch.equal(maps[at].view(torch.int32), one[0].view(torch.int32))
    utils.set_cur_iter(1)


def test_two_bands_sum_to_the_one_rank_map_and_gradients_are_refused(device):
    import gaussian_renderer as gr
    import gaussian_renderer.workload_division as wd
    import utils.general_utils as utils
    from fake_world import FakeWorld

    world = 2
    fw = FakeWorld(world, device)

    def rank_main(rank):
        utils.GLOBAL_RANK, utils.LOCAL_RANK, utils.WORLD_SIZE = rank, 0, world
        utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = fw.groups[rank]
        utils.set_args(utils.default_args(bsz=1, no_heuristics_update=True))
        utils.set_img_size(H, W)
        utils.set_cur_iter(1)
        wd._BALANCE["mode"] = "exact"
        gr._PLANNERS.clear()
        model = S.SyntheticGaussianModel(N, W, H, seed=SEED, sh_degree=DEG, rank=rank, world_size=world, device=device,
                                         scale_coef=SCALE)
        image, inv, pkg = _render_rank(model, device, world, rank)
        collectives = len(fw.log)  # (every collective of the forward is a rendezvous both ranks have passed)
        refused = False
        if inv is not None and inv.requires_grad:
            try:
                inv.sum().backward()
            except NotImplementedError:
                refused = True
        return dict(inv=None if inv is None else inv.detach().clone(), refused=refused,
                    grads=[getattr(model, n).grad for n in ALL], collectives=(collectives, len(fw.log)))

    gr.set_invdepth(True)
    try:
        res = fw.run(rank_main, timeout=120)
    finally:
        gr.set_invdepth(False)
    assert all(r["inv"] is not None for r in res), "a rank rendered no band of the camera"
    assert all(r["refused"] for r in res), "the map's gradient at world size 2 was not refused"
    assert all(g is None for r in res for g in r["grads"]), "a gradient arrived although the backward was refused"
    assert all(r["collectives"][0] == r["collectives"][1] == len(fw.log) for r in res), \
        f"a collective ran behind the forward: {fw.log}"
    _single_rank(device)
    with torch.no_grad():
        _, one, _ = _render(_model(device), device, True, mode="test")
    total = res[0]["inv"] + res[1]["inv"]
    assert bool(res[0]["inv"].any()) and bool(res[1]["inv"].any()), "a band's map is empty: the sum shows nothing"
    assert not bool(((res[0]["inv"] != 0) & (res[1]["inv"] != 0)).any()), "the bands overlap"
    assert torch.equal(total.view(torch.int32), one.view(torch.int32)), "the bands do not SUM to the one-rank map"


def _render_rank(model, dev, world, rank):
    """one fake rank's two calls (the switch is on for the whole fake world: the ranks share the module)"""
    from gaussian_renderer import distributed_preprocess3dgs_and_all2all_final, render_final
    from gaussian_renderer.workload_division import DivisionStrategyHistoryFinal, start_strategy_final

    cams = S.orbit_cameras(4, W, H, device=dev)
    hist = DivisionStrategyHistoryFinal(S.SyntheticDataset(cams), world, rank)
    strategies, _ = start_strategy_final([cams[VIEW]], hist)
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    pipe = type("P", (), {"debug": False})()
    pkg = distributed_preprocess3dgs_and_all2all_final([cams[VIEW]], model, pipe, bg, batched_strategies=strategies,
                                                       mode="train")
    images, _ = render_final(pkg, strategies)
    return images[0], pkg["batched_invdepth"][0], pkg
