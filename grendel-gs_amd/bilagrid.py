"""Bilateral-grid colour correction: one learned lattice G[12, L, GH, GW] of [3,4] affine colour transforms per training
image, sampled per pixel at (position in the image, luminance of the rendered colour).

A global [3,4] exposure (exposure.py) cannot absorb what varies across the frame or with brightness -- vignetting, the
local tone mapping of phone and drone ISPs, white balance that reacts to the sky, highlight roll-off.  The grid can
(Wang et al., "Bilateral Guided Radiance Field Processing"; gsplat's `use_bilateral_grid`), and contains the exposure's
affine transform as the special case of equal nodes.  The rendered band is passed through the slice kernel
(include/gsraster.h, N1g; diff_gaussian_rasterization.bilagrid_slice) in front of the loss, and the grids are
regularised by their total variation.  The reference has no such model: the definition is this project's (DESIGN.md
3.15).

    model = BilateralGridModel(len(train_cameras))
    loss_distribution.set_bilateral_grid(model)    # batched_loss_computation now corrects with camera.uid's grid
    ...  loss.backward()
    model.sync_grads(utils.DEFAULT_GROUP)          # ONE collective per step: every rank holds a partial gradient
    model.step()                                   # + tv_weight * dT/dG (one launch), dense Adam over all rows (one launch)

The parameter is replicated on every rank.  Evaluation stays uncorrected (test views have no learned grid).
"""
import torch
import torch.distributed as dist


def apply_bilagrid(image, grid):
    """x' = A_M c + b_M of a full image [3,H,W] under one grid [12,L,GH,GW], in torch (grid_sample on the 5-D lattice): for
    callers that export or inspect a corrected training view.  The loss never calls this: it runs the slice kernel, whose
    definition -- the lower node, a + t (b - a) per axis -- this agrees with up to rounding."""
    if image.dim() != 3 or image.shape[0] != 3 or grid.dim() != 4 or grid.shape[0] != 12:
        raise ValueError(f"apply_bilagrid: needs a [3,H,W] image and a [12,L,GH,GW] grid, got {tuple(image.shape)} and "
                         f"{tuple(grid.shape)}")
    _, H, W = image.shape
    grid = grid.to(image.dtype)
    u = ((torch.arange(W, device=image.device, dtype=image.dtype) + 0.5) / W).expand(H, W)
    v = ((torch.arange(H, device=image.device, dtype=image.dtype) + 0.5) / H)[:, None].expand(H, W)
    lum = (0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]).clamp(0, 1)
    coords = torch.stack([u, v, lum], dim=-1) * 2 - 1  # (x, y, z) in [-1, 1]
    M = torch.nn.functional.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True,
                                        padding_mode="border")[0, :, 0].reshape(3, 4, H, W)
    return (M[:, :3] * image[None]).sum(dim=1) + M[:, 3]


class BilateralGridModel:
    """[N, 12, L, GH, GW] grids (`grid` = (GW, GH, L)), every node initialised to [I | 0], with their own dense Adam whose
    learning rate decays exponentially: update number k (1-based) runs at lr_at(k),
    lr_at(t) = lr_init * (lr_final / lr_init) ** (min(t, max_steps) / max_steps).  step() adds tv_weight * dT/dG, T the
    total variation of all grids (include/gsraster.h, N1g), to the gradient before the update.

    The defaults (grid, learning rates, tv_weight = 10, eps = 1e-15) are gsplat's as far as remembered; nothing in this
    project has tuned them."""

    def __init__(self, num_cameras, grid=(16, 16, 8), lr_init=2e-3, lr_final=2e-5, max_steps=30000, tv_weight=10.0,
                 betas=(0.9, 0.999), eps=1e-15, device="cuda"):
        if num_cameras <= 0:
            raise ValueError("BilateralGridModel: num_cameras must be positive")
        if not (lr_init > 0 and lr_final > 0 and max_steps > 0):
            raise ValueError("BilateralGridModel: lr_init, lr_final and max_steps must be positive")
        gw, gh, gl = (int(s) for s in grid)
        if not (2 <= gw <= 64 and 2 <= gh <= 64 and 2 <= gl <= 16):
            raise ValueError(f"BilateralGridModel: grid (GW, GH, L) = {(gw, gh, gl)} outside 2..64, 2..64, 2..16")
        if tv_weight < 0:
            raise ValueError("BilateralGridModel: tv_weight must not be negative")
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1).reshape(12)
        self.grids = eye[None, :, None, None, None].expand(num_cameras, 12, gl, gh, gw).contiguous().to(device)
        self.grids.requires_grad_(True)
        self.exp_avg = torch.zeros_like(self.grids, requires_grad=False)
        self.exp_avg_sq = torch.zeros_like(self.grids, requires_grad=False)
        self.lr_init, self.lr_final, self.max_steps = float(lr_init), float(lr_final), int(max_steps)
        self.tv_weight = float(tv_weight)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0  # updates made so far

    @property
    def num_cameras(self):
        return int(self.grids.shape[0])

    def of(self, camera):
        """the [12, L, GH, GW] grid of `camera` (row camera.uid): a differentiable view of the parameter"""
        uid = int(camera.uid)
        if not 0 <= uid < self.num_cameras:
            raise IndexError(f"BilateralGridModel: camera uid {uid} outside [0, {self.num_cameras})")
        return self.grids[uid]

    def lr_at(self, t):
        f = min(max(int(t), 0), self.max_steps) / self.max_steps
        return self.lr_init * (self.lr_final / self.lr_init) ** f

    def sync_grads(self, group=None):
        """SUM all-reduce of the gradient over `group` when it has more than one rank: every rank that rendered a band of
        a camera holds a partial gradient of that camera's grid.  One collective per step for the whole batch (a rank
        that rendered nothing contributes zeros).  The total-variation term is added by step(), after this."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        if self.grids.grad is None:
            self.grids.grad = torch.zeros_like(self.grids)
        dist.all_reduce(self.grids.grad, op=dist.ReduceOp.SUM, group=group)

    def zero_grad(self):
        self.grids.grad = None

    def step(self):
        """tv_weight * dT/dG added to the gradient (one launch: gsr_bilagrid_tv; every rank adds the same thing to its
        all-reduced gradient), then one dense Adam update of all rows in ONE launch (gsr_adam_step), then the gradient
        is dropped.  Without a gradient nothing happens (and the step count stays)."""
        g = self.grids.grad
        if g is None:
            return
        if not self.grids.is_cuda:
            raise RuntimeError("BilateralGridModel.step: the parameter must live on the gfx950 device (there is no CPU "
                               "path)")
        import diff_gaussian_rasterization as dgr

        g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        if self.tv_weight > 0:
            dgr.bilagrid_tv(self.grids, self.tv_weight, grad=g)
        self.steps += 1
        with dgr._on(self.grids.device):
            dgr.check(dgr.lib.gsr_adam_step(self.grids.numel(), self.grids.data_ptr(), g.data_ptr(),
                                            self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.lr_at(self.steps),
                                            self.betas[0], self.betas[1], self.eps, self.steps, 1.0, dgr._stream()),
                      "gsr_adam_step")
        self.grids.grad = None

    def state_dict(self):
        return dict(grids=self.grids.detach().clone(), exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(),
                    steps=self.steps)

    def load_state_dict(self, state):
        for name in ("grids", "exp_avg", "exp_avg_sq"):
            t = state[name]
            if tuple(t.shape) != tuple(self.grids.shape):
                raise ValueError(f"BilateralGridModel.load_state_dict: {name} has shape {tuple(t.shape)}, expected "
                                 f"{tuple(self.grids.shape)}")
        with torch.no_grad():
            self.grids.copy_(state["grids"])
            self.exp_avg.copy_(state["exp_avg"])
            self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.steps = int(state["steps"])
        self.grids.grad = None
