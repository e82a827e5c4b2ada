"""Per-camera exposure compensation: one learned [3,4] colour transform E = [A | b] per training image.

Outdoor captures vary in exposure and white balance from frame to frame; without a per-image transform the Gaussians absorb
the brightness differences as floaters.  The loss of a rendered band is taken on x' = A x + b (no clamp) inside the fused
L1 + SSIM kernels (include/gsraster.h, N1x; diff_gaussian_rasterization.fused_band_loss_exposure), which also reduce the
12 gradient sums of E -- nothing of this runs as torch glue around the loss.  The reference has no exposure model: the
definition is this project's, the idea is upstream 3DGS's "exposure compensation".

    model = ExposureModel(len(train_cameras))
    loss_distribution.set_exposure_model(model)    # batched_loss_computation now compensates camera.uid's row
    ...  loss.backward()
    model.sync_grads(utils.DEFAULT_GROUP)          # ONE collective per step: every rank holds a partial gradient
    model.step()                                   # dense Adam over all N rows, one launch (gsr_adam_step)

The parameter is replicated on every rank.  Evaluation stays uncompensated (test views have no learned exposure).
"""
import torch
import torch.distributed as dist


def apply_exposure(image, E):
    """x' = A x + b of a full image [3,H,W] with E = [A | b] ([3,4]), in torch: for callers that export or inspect a
    compensated training view (the loss never calls this: it forms x' inside its kernels)"""
    E = E.to(image.dtype)
    return torch.einsum("ck,khw->chw", E[:, :3], image) + E[:, 3, None, None]


class ExposureModel:
    """[N,3,4] exposures, initialised to [I | 0], with their own dense Adam (betas / eps as given) whose learning rate
    decays exponentially: update number k (1-based, the Adam step count) runs at lr_at(k),
    lr_at(t) = lr_init * (lr_final / lr_init) ** (min(t, max_steps) / max_steps)."""

    def __init__(self, num_cameras, lr_init=0.01, lr_final=0.001, max_steps=30000, device="cuda", betas=(0.9, 0.999),
                 eps=1e-8):
        if num_cameras <= 0:
            raise ValueError("ExposureModel: num_cameras must be positive")
        if not (lr_init > 0 and lr_final > 0 and max_steps > 0):
            raise ValueError("ExposureModel: lr_init, lr_final and max_steps must be positive")
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
        self.exposure = eye.expand(num_cameras, 3, 4).contiguous().to(device).requires_grad_(True)
        self.exp_avg = torch.zeros_like(self.exposure, requires_grad=False)
        self.exp_avg_sq = torch.zeros_like(self.exposure, requires_grad=False)
        self.lr_init, self.lr_final, self.max_steps = float(lr_init), float(lr_final), int(max_steps)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0  # updates made so far

    @property
    def num_cameras(self):
        return int(self.exposure.shape[0])

    def of(self, camera):
        """the [3,4] exposure of `camera` (row camera.uid): a differentiable view of the parameter"""
        uid = int(camera.uid)
        if not 0 <= uid < self.num_cameras:
            raise IndexError(f"ExposureModel: camera uid {uid} outside [0, {self.num_cameras})")
        return self.exposure[uid]

    def lr_at(self, t):
        f = min(max(int(t), 0), self.max_steps) / self.max_steps
        return self.lr_init * (self.lr_final / self.lr_init) ** f

    def sync_grads(self, group=None):
        """SUM all-reduce of the gradient over `group` when it has more than one rank: every rank that rendered a band of
        a camera holds a partial gradient of that camera's row.  One collective per step for the whole batch (a rank that
        rendered nothing contributes zeros)."""
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) <= 1:
            return
        if self.exposure.grad is None:
            self.exposure.grad = torch.zeros_like(self.exposure)
        dist.all_reduce(self.exposure.grad, op=dist.ReduceOp.SUM, group=group)

    def zero_grad(self):
        self.exposure.grad = None

    def step(self):
        """one dense Adam update of all N rows in ONE launch (include/gsraster.h: gsr_adam_step), then the gradient is
        dropped.  Without a gradient nothing happens (and the step count stays)."""
        g = self.exposure.grad
        if g is None:
            return
        if not self.exposure.is_cuda:
            raise RuntimeError("ExposureModel.step: the parameter must live on the gfx950 device (there is no CPU path)")
        import diff_gaussian_rasterization as dgr

        g = g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()
        self.steps += 1
        with dgr._on(self.exposure.device):
            dgr.check(dgr.lib.gsr_adam_step(self.exposure.numel(), self.exposure.data_ptr(), g.data_ptr(),
                                            self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.lr_at(self.steps),
                                            self.betas[0], self.betas[1], self.eps, self.steps, 1.0, dgr._stream()),
                      "gsr_adam_step")
        self.exposure.grad = None

    def state_dict(self):
        return dict(exposure=self.exposure.detach().clone(), exp_avg=self.exp_avg.clone(),
                    exp_avg_sq=self.exp_avg_sq.clone(), steps=self.steps)

    def load_state_dict(self, state):
        for name in ("exposure", "exp_avg", "exp_avg_sq"):
            t = state[name]
            if tuple(t.shape) != tuple(self.exposure.shape):
                raise ValueError(f"ExposureModel.load_state_dict: {name} has shape {tuple(t.shape)}, expected "
                                 f"{tuple(self.exposure.shape)}")
        with torch.no_grad():
            self.exposure.copy_(state["exposure"])
            self.exp_avg.copy_(state["exp_avg"])
            self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.steps = int(state["steps"])
        self.exposure.grad = None
