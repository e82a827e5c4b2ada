"""Fixed-budget densification: 3DGS-MCMC ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy) on
the kernels of csrc/mcmc.hip.  Opt-in; the reference has none of it and nothing here changes a default.

* relocate_and_grow: dead Gaussians (opacity <= min_opacity) are teleported IN PLACE onto live ones drawn in proportion to
  opacity, and the population grows by `grow_factor` per event up to `cap_max`, the new rows being drawn the same way.
  The source's opacity and scale are corrected so that the rendered image does not change.  Rows live in a RowArena of
  capacity cap_max: nothing moves, nothing is allocated after the first event, and NOTHING is read back to the host --
  the number of new rows follows from the row count alone.
* inject_noise: xyz += noise_lr * xyz_lr * gate(1 - opacity) * Sigma * xi after every optimizer step, one launch.
* add_regulariser_grads: the closed-form gradients of opacity_reg * mean(opacity) + scale_reg * mean(scale), added to
  `.grad` in one launch.  Not available with FusedAdam(fuse_backward=True): the gradients never reach memory there.

Once the budget is reached the row count stays constant: no Parameter object changes in an event, the optimizer is not
re-keyed, and in a sharded run (cap_max is PER RANK, every step is shard-local, no communication) the shards stop
drifting apart, so redistribution is no longer needed.

Determinism: every draw is a pure function of (seed, rank, iteration, row) -- Philox4x32-10 on the device -- so the same
seed, event and step give the same bits whatever the launch geometry.
"""
import torch
import torch.distributed as dist

import densification_ops as D
import diff_gaussian_rasterization as dgr

_MASK64 = (1 << 64) - 1
_ROLE = {"opacity": dgr.MCMC_ROLE_OPACITY, "scaling": dgr.MCMC_ROLE_SCALING}


def _mix_rank(seed, rank):
    """the device seed of `rank`: splitmix64 of seed + rank * golden ratio (rank 0 of seed s differs from rank 1 of s-1)"""
    z = (int(seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


class MCMCStrategy:
    def __init__(self, cap_max, min_opacity=0.005, noise_lr=5e5, opacity_reg=0.01, scale_reg=0.01, grow_factor=1.05,
                 n_max=51, seed=0, rank=None):
        if int(cap_max) < 1 or not 1 <= int(n_max) <= dgr.MCMC_N_MAX or not grow_factor >= 1.0:
            raise ValueError("MCMCStrategy: cap_max >= 1, 1 <= n_max <= 51 and grow_factor >= 1 expected")
        self.cap_max, self.min_opacity, self.noise_lr = int(cap_max), float(min_opacity), float(noise_lr)
        self.opacity_reg, self.scale_reg, self.grow_factor = float(opacity_reg), float(scale_reg), float(grow_factor)
        self.n_max, self.seed, self.rank = int(n_max), int(seed), rank
        self.totals = None  # device int64 [2] of the last event: {n_dead, n_alive}; never read here

    def device_seed(self):
        rank = self.rank
        if rank is None:
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        return _mix_rank(self.seed, rank)

    def rows_after(self, P):
        """the row count after an event on P rows: min(cap_max, int(grow_factor * P)), never fewer than P"""
        return max(P, min(self.cap_max, int(self.grow_factor * P)))

    @torch.no_grad()
    def relocate_and_grow(self, model, iteration):
        """one event; returns the number of rows added (host arithmetic, no read-back)"""
        P = model._xyz.shape[0]
        n_new = self.rows_after(P)
        n_add = n_new - P
        arena = D.row_arena(model, capacity=self.cap_max)
        opacity_act = model.get_opacity.detach().reshape(-1).contiguous()  # the model's own getter, as densify_classes
        slots = D._optimizer_slots(model)
        tensors = [D._slot_tensor(model, g, k).detach() for g, k in slots]
        keys = [(g["name"], k) for g, k in slots]
        roles = [dgr.MCMC_ROLE_MOMENT if k is not None else _ROLE.get(g["name"], dgr.MCMC_ROLE_COPY) for g, k in slots]
        cnt = getattr(model, "send_to_gpui_cnt", None)
        if cnt is not None:
            tensors.append(cnt)
            keys.append(("send_to_gpui_cnt", None))
            roles.append(dgr.MCMC_ROLE_COPY)
        if n_add > 0:
            # the longer views of the same arena rows (the first event copies the model's tensors in, once); new rows
            # start as zeros, which is what they stay if no live row exists to draw from
            tensors = [arena.extend(key, t.contiguous(), n_new) for key, t in zip(keys, tensors)]
            for t in tensors:
                t[P:].zero_()
        src, count, self.totals = dgr.mcmc_relocate_plan(
            opacity_act, n_add, self.min_opacity, self.device_seed(), iteration,
            arena.scratch("mcmc_src", max(n_new, arena.capacity), torch.int32),
            arena.scratch("mcmc_count", max(P, arena.capacity), torch.int32),
            arena.scratch("mcmc_plan", (dgr.lib.gsr_mcmc_relocate_bytes(max(P, arena.capacity)) + 7) // 8, torch.int64))
        dgr.mcmc_relocate_apply(src, count, opacity_act, self.min_opacity, tensors, roles, self.n_max)
        if n_add > 0:
            D._replace_optimizer_rows(model, slots, tensors[:len(slots)])
            if cnt is not None:
                model.send_to_gpui_cnt = tensors[-1]
        model.xyz_gradient_accum = arena.zeros("xyz_gradient_accum", n_new, (1,))
        model.denom = arena.zeros("denom", n_new, (1,))
        model.max_radii2D = arena.zeros("max_radii2D", n_new)
        model.sum_visible_count_in_one_batch = arena.zeros("sum_visible_count_in_one_batch", n_new)
        arena.events += 1
        return n_add

    @torch.no_grad()
    def inject_noise(self, model, iteration, xyz_lr):
        """call after optimizer.step(): the positions move by noise_lr * xyz_lr * gate * Sigma * xi, in place"""
        dgr.mcmc_noise(model._xyz.data, model._scaling.data, model._rotation.data, model._opacity.data,
                       self.noise_lr * float(xyz_lr), None, self.device_seed(), iteration)

    @torch.no_grad()
    def add_regulariser_grads(self, model, count=None):
        """call between backward and optimizer.step(): adds the gradients of opacity_reg * mean(get_opacity) + scale_reg *
        mean(get_scaling) to _opacity.grad / _scaling.grad.  count: the number of Gaussians the means run over (default:
        this model's rows; a sharded run passes the global count)."""
        if getattr(model.optimizer, "fuse_backward", False):
            raise ValueError("MCMCStrategy.add_regulariser_grads needs an optimizer with fuse_backward=False: the fused "
                             "K11 + Adam step never writes the gradients the regulariser is added to")
        P = model._xyz.shape[0]
        count = P if count is None else int(count)
        if model._opacity.grad is None or model._scaling.grad is None:
            raise ValueError("MCMCStrategy.add_regulariser_grads: call after backward (no .grad to add to)")
        dgr.mcmc_reg_grad(model._opacity.data, model._scaling.data, self.opacity_reg / count,
                          self.scale_reg / (3 * count), model._opacity.grad, model._scaling.grad)


def install(cls):
    """graft: GaussianModel.mcmc_relocate_and_grow / mcmc_inject_noise / mcmc_add_regulariser_grads, which act through
    the MCMCStrategy stored as `self.mcmc_strategy`"""
    def mcmc_relocate_and_grow(self, iteration):
        return self.mcmc_strategy.relocate_and_grow(self, iteration)

    def mcmc_inject_noise(self, iteration, xyz_lr):
        return self.mcmc_strategy.inject_noise(self, iteration, xyz_lr)

    def mcmc_add_regulariser_grads(self, count=None):
        return self.mcmc_strategy.add_regulariser_grads(self, count)

    for fn in (mcmc_relocate_and_grow, mcmc_inject_noise, mcmc_add_regulariser_grads):
        setattr(cls, fn.__name__, fn)
    return cls
