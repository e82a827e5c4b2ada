"""N4 -- densification / redistribution of the Gaussian shard on top of the row primitives of libgsraster.so.

Host-side mirror of the GaussianModel methods the reference's densification step calls
(densification.py:5-86 -> scene/gaussian_model.py): `prune_points` (:835-852, `_prune_optimizer` :793-818),
`densification_postfix` / `cat_tensors_to_optimizer` (:854-921), `densify_and_clone` (:972-1005),
`densify_and_split` (:922-970), `densify_and_prune` (:1007-1044) and `redistribute_gaussians` (:1264-1329).
Same names, arguments, semantics and optimizer-state surgery; what changes is HOW rows are moved:

* the reference evaluates `tensor[mask]` once per tensor (6 parameters + 12 Adam moments + 5 statistics; each a
  `nonzero` host sync + an index kernel) and, for redistribution, once per tensor PER DESTINATION RANK followed
  by 18 separate all-to-alls;
* here the selection is computed once (`group_rows`, one radix pass, one host read-back) and applied to all
  tensors in one launch (`gather_rows`); redistribution packs every per-Gaussian tensor into one record matrix
  and issues ONE all-to-all-v over RCCL (the reference's disabled "implementation_2", :1206-1238).

Every function takes the model as its first argument, so `install(GaussianModel)` makes them the methods of the
reference's own class (graft level B3).  The model duck type: the six raw parameters `_xyz,
_features_dc, _features_rest, _opacity, _scaling, _rotation`, `optimizer` (one group per parameter, named
xyz / f_dc / f_rest / opacity / scaling / rotation), the statistics `xyz_gradient_accum, denom, max_radii2D,
sum_visible_count_in_one_batch, send_to_gpui_cnt`, `percent_dense`, and the getters.
There is no CPU fallback: the tensors live on the gfx950 device.

Opt-in (`GSR_FUSED_DENSIFY=1` or `set_fused_densify(True)`): `densify_and_prune` as ONE pass over reserved row storage
-- `densify_and_prune_fused` below, DESIGN.md "One-pass densification".
"""
import math
import os

import torch
import torch.distributed as dist
from torch import nn

import diff_gaussian_rasterization as dgr
import utils.general_utils as utils
from row_arena import RowArena

_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
         "scaling": "_scaling", "rotation": "_rotation"}
_STATS = ["xyz_gradient_accum", "denom", "max_radii2D", "sum_visible_count_in_one_batch", "send_to_gpui_cnt"]


def _log(msg):
    f = utils.get_log_file() if hasattr(utils, "get_log_file") else None
    if f is not None:
        f.write(msg)


def _optimizer_slots(self):
    """[(group, key)] for every per-Gaussian tensor the optimizer holds; key None = the parameter itself"""
    slots = []
    for group in self.optimizer.param_groups:
        assert len(group["params"]) == 1
        st = self.optimizer.state.get(group["params"][0], None)
        if st is not None:
            for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
                if key in st:
                    slots.append((group, key))
        slots.append((group, None))
    return slots


def _slot_tensor(self, group, key):
    p = group["params"][0]
    return p.data if key is None else self.optimizer.state[p][key]


def _replace_optimizer_rows(self, slots, new_tensors):
    """the optimizer-state surgery of _prune_optimizer / cat_tensors_to_optimizer / update_all_optimizer_states
    (scene/gaussian_model.py:793-818,854-893,1175-1204): new Parameter objects, state re-keyed"""
    new = {(id(g), k): t for (g, k), t in zip(slots, new_tensors)}
    out = {}
    for group in self.optimizer.param_groups:
        old = group["params"][0]
        st = self.optimizer.state.get(old, None)
        if st is not None:
            for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
                if key in st:
                    st[key] = new[(id(group), key)]
            del self.optimizer.state[old]
        group["params"][0] = nn.Parameter(new[(id(group), None)].requires_grad_(True))
        if st is not None:
            self.optimizer.state[group["params"][0]] = st
        out[group["name"]] = group["params"][0]
    for name, attr in _ATTR.items():
        setattr(self, attr, out[name])
    return out


def _live_stats(self):
    return [n for n in _STATS if getattr(self, n, None) is not None]


# ----------------------------------------------------------------------------------------- prune
def prune_points(self, mask):
    """drop the rows where `mask` is True from the 6 parameters, their Adam moments and the statistics"""
    dest = mask.to(torch.int32).neg()  # keep -> group 0, prune -> dropped
    order, counts = dgr.group_rows(dest, 1)
    n = counts[0]
    slots = _optimizer_slots(self)
    stats = _live_stats(self)
    srcs = [_slot_tensor(self, g, k) for g, k in slots] + [getattr(self, s) for s in stats]
    outs = dgr.gather_rows(order, n, srcs)
    _replace_optimizer_rows(self, slots, outs[:len(slots)])
    for s, t in zip(stats, outs[len(slots):]):
        setattr(self, s, t)


# ------------------------------------------------------------------------------------- densify
def cat_tensors_to_optimizer(self, tensors_dict):
    slots = _optimizer_slots(self)
    new = []
    for g, k in slots:
        ext = tensors_dict[g["name"]]
        cur = _slot_tensor(self, g, k)
        new.append(torch.cat((cur, ext if k is None else torch.zeros_like(ext)), dim=0))
    return _replace_optimizer_rows(self, slots, new)


def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling,
                          new_rotation, new_send_to_gpui_cnt):
    cat_tensors_to_optimizer(self, {"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest,
                                    "opacity": new_opacities, "scaling": new_scaling, "rotation": new_rotation})
    n, dev = self._xyz.shape[0], self._xyz.device
    self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    self.denom = torch.zeros((n, 1), device=dev)
    self.max_radii2D = torch.zeros((n,), device=dev)
    self.sum_visible_count_in_one_batch = torch.zeros((n,), device=dev)
    if getattr(self, "send_to_gpui_cnt", None) is not None:
        self.send_to_gpui_cnt = torch.cat((self.send_to_gpui_cnt, new_send_to_gpui_cnt), dim=0)


def _selected_rows(self, selected_pts_mask, names):
    """rows of the named attributes where the mask is True: one grouping + one gather launch"""
    order, counts = dgr.group_rows(selected_pts_mask.to(torch.int32) - 1, 1)  # True -> 0, False -> -1
    srcs = [getattr(self, n).data if isinstance(getattr(self, n), nn.Parameter) else getattr(self, n) for n in names]
    return counts[0], dgr.gather_rows(order, counts[0], srcs)


def _build_rotation(r):
    """utils/general_utils.py:416-439 of the reference"""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def densify_and_clone(self, grads, grad_threshold, scene_extent):
    sel = torch.norm(grads, dim=-1) >= grad_threshold
    sel = torch.logical_and(sel, torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    has_cnt = getattr(self, "send_to_gpui_cnt", None) is not None
    n, rows = _selected_rows(self, sel, names + (["send_to_gpui_cnt"] if has_cnt else []))
    _log("Number of cloned gaussians: {}\n".format(n))
    densification_postfix(self, *rows[:6], rows[6] if has_cnt else None)


def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
    n_init = self._xyz.shape[0]
    padded_grad = torch.zeros((n_init,), device=self._xyz.device)
    padded_grad[: grads.shape[0]] = grads.squeeze()
    sel = padded_grad >= grad_threshold
    sel = torch.logical_and(sel, torch.max(self.get_scaling, dim=1).values > self.percent_dense * scene_extent)
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    has_cnt = getattr(self, "send_to_gpui_cnt", None) is not None
    n, rows = _selected_rows(self, sel, names + (["send_to_gpui_cnt"] if has_cnt else []))
    xyz, f_dc, f_rest, opacity, scaling_raw, rotation = rows[:6]
    _log("Number of split gaussians: {}\n".format(n))
    scaling = torch.exp(scaling_raw)  # get_scaling of the selected rows
    stds = scaling.repeat(N, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=stds.device), std=stds)
    rots = _build_rotation(rotation).repeat(N, 1, 1)
    new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + xyz.repeat(N, 1)
    new_scaling = torch.log(scaling.repeat(N, 1) / (0.8 * N))
    densification_postfix(self, new_xyz, f_dc.repeat(N, 1, 1), f_rest.repeat(N, 1, 1), opacity.repeat(N, 1),
                          new_scaling, rotation.repeat(N, 1), rows[6].repeat(N, 1) if has_cnt else None)
    prune_filter = torch.cat((sel, torch.zeros(N * n, device=sel.device, dtype=torch.bool)))
    prune_points(self, prune_filter)


def _sync_replicated_statistics(self):
    args = utils.get_args()
    if not getattr(args, "gaussians_distribution", True) and utils.DEFAULT_GROUP.size() > 1:
        # replicated storage (scene/gaussian_model.py:1006-1016): every rank saw only its own pixels, so the replicas
        # agree on the statistics first -- otherwise they would clone / split / prune different sets and diverge
        group = getattr(utils, "DP_GROUP", None) or utils.DEFAULT_GROUP
        dist.all_reduce(self.max_radii2D, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(self.xyz_gradient_accum, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self.denom, op=dist.ReduceOp.SUM, group=group)


def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
    if fused_densify_enabled():
        return densify_and_prune_fused(self, max_grad, min_opacity, extent, max_screen_size)
    _sync_replicated_statistics(self)
    _densify_and_prune_steps(self, max_grad, min_opacity, extent, max_screen_size)


def _densify_and_prune_steps(self, max_grad, min_opacity, extent, max_screen_size):
    """clone, split, prune one after the other, as the reference orders them"""
    grads = self.xyz_gradient_accum / self.denom
    grads[grads.isnan()] = 0.0
    densify_and_clone(self, grads, max_grad, extent)
    densify_and_split(self, grads, max_grad, extent)
    prune_mask = (self.get_opacity < min_opacity).squeeze()
    if max_screen_size:
        big_points_vs = self.max_radii2D > max_screen_size
        big_points_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
    prune_points(self, prune_mask)


# ------------------------------------------------------------------------ one-pass densification
# The clone -> split -> prune sequence above has a closed-form result in terms of the ORIGINAL rows (DESIGN.md
# "One-pass densification"): [kept originals | kept clones | first children | second children], original order inside
# each segment.  The rows are classified with the model's own getters (plain torch, any device), ranked by one scan
# (gsr_densify_plan), and written for all tensors by one launch (gsr_densify_move) from one half of a RowArena into the
# other: no torch.cat, no boolean indexing, one host read-back.
_FUSED = [None]  # None: the environment decides


def set_fused_densify(on):
    """True / False: densify_and_prune takes / does not take the one-pass path; None: GSR_FUSED_DENSIFY decides"""
    _FUSED[0] = None if on is None else bool(on)


def fused_densify_enabled():
    if _FUSED[0] is not None:
        return _FUSED[0]
    return os.environ.get("GSR_FUSED_DENSIFY", "0") not in ("", "0")  # read at call time


def densify_classes(self, max_grad, min_opacity, extent, max_screen_size, N=2):
    """-> (cls uint8 [P], child_scaling [P,3], get_scaling [P,3]): what the reference's densify_and_prune does to every ORIGINAL row, in the
    expressions of densify_and_clone / densify_and_split / densify_and_prune applied to the model's own getters
    (scene/gaussian_model.py:922-1044), so the selection is the reference's whatever the activations are.
    Bits: 1 the original stays, 2 a clone is appended, 4 the row is split, 8 its children survive the final prune.
    child_scaling = scaling_inverse_activation(get_scaling / (0.8 N)), the children's raw scale (:940), through the
    model's own inverse activation / activation where it names them (log / exp otherwise).  The final prune's
    `max_radii2D > max_screen_size` never fires (densification_postfix zeroes max_radii2D first) and is left out;
    clones carry gradient 0 in the split step, so they are never split for max_grad > 0 (the caller's precondition)."""
    grads = self.xyz_gradient_accum / self.denom
    grads[grads.isnan()] = 0.0
    scaling = self.get_scaling
    s = torch.max(scaling, dim=1).values
    clone = torch.logical_and(torch.norm(grads, dim=-1) >= max_grad, s <= self.percent_dense * extent)
    split = torch.logical_and(grads.reshape(-1) >= max_grad, s > self.percent_dense * extent)
    child_scaling = getattr(self, "scaling_inverse_activation", torch.log)(scaling / (0.8 * N))
    drop = (self.get_opacity < min_opacity).reshape(-1)
    drop_child = drop
    if max_screen_size:
        # the getter's view of the children's new raw parameter: the model's own activation where it names one
        act = getattr(self, "scaling_activation", torch.exp)
        drop_child = torch.logical_or(drop, act(child_scaling).max(dim=1).values > 0.1 * extent)
        drop = torch.logical_or(drop, s > 0.1 * extent)
    keep, keep_child = ~drop, ~drop_child
    cls = (~split & keep).to(torch.uint8)
    cls += (clone & keep).to(torch.uint8) * 2
    cls += split.to(torch.uint8) * 4
    cls += (split & keep_child).to(torch.uint8) * 8
    return cls, child_scaling, scaling


def _has_adam_state(self):
    for group in self.optimizer.param_groups:
        st = self.optimizer.state.get(group["params"][0], None)
        if st is None or "exp_avg" not in st or "exp_avg_sq" not in st:
            return False
    return True


def row_arena(self, capacity=None):
    """the model's RowArena, created at the first one-pass event (or here, e.g. with an explicit capacity)"""
    arena = getattr(self, "_row_arena", None)
    if arena is None:
        arena = self._row_arena = RowArena(self._xyz.shape[0], self._xyz.device, capacity)
    return arena


_ROLE = {"xyz": dgr.DENSIFY_ROLE_XYZ, "scaling": dgr.DENSIFY_ROLE_SCALING}


@torch.no_grad()
def densify_and_prune_fused(self, max_grad, min_opacity, extent, max_screen_size, N=2):
    """densify_and_prune (scene/gaussian_model.py:1007-1044) as one pass: same arguments, same result -- bit for bit,
    except that a child's position is R . sample + xyz evaluated by the move kernel instead of torch.bmm (a few ulp).
    Falls back to the step-by-step path when max_grad <= 0 (clones could then be split) or the optimizer has no Adam
    moments yet."""
    _sync_replicated_statistics(self)
    if not max_grad > 0 or not _has_adam_state(self):
        return _densify_and_prune_steps(self, max_grad, min_opacity, extent, max_screen_size)
    cls, child_scaling, scaling = densify_classes(self, max_grad, min_opacity, extent, max_screen_size, N)
    P, dev = cls.shape[0], cls.device
    arena = row_arena(self)
    cap = max(P, arena.capacity)  # (the plan's buffers are reserved for the capacity, like the rows)
    ranks, split_rows, counts = dgr.densify_plan(
        cls, arena.scratch("ranks", 4 * cap, torch.int32), arena.scratch("split_rows", cap, torch.int32),
        arena.scratch("plan", dgr.lib.gsr_densify_plan_bytes(cap), torch.uint8))
    n_orig, n_clone, n_child, n_split = counts.cpu().tolist()  # THE host read-back of the event
    _log("Number of cloned gaussians kept: {}\n".format(n_clone))
    _log("Number of split gaussians: {}\n".format(n_split))
    # the reference's draw (:933-936), same call on the same device -> the same bits: the standard deviations are the
    # scales of the split rows in row order, repeated N times
    stds = scaling.index_select(0, split_rows[:n_split]).repeat(N, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
    n_new = n_orig + n_clone + N * n_child
    slots = _optimizer_slots(self)
    srcs = [_slot_tensor(self, g, k) for g, k in slots]
    keys = [(g["name"], k) for g, k in slots]
    roles = [dgr.DENSIFY_ROLE_MOMENT if k is not None else _ROLE.get(g["name"], dgr.DENSIFY_ROLE_COPY) for g, k in slots]
    alts = [child_scaling if r == dgr.DENSIFY_ROLE_SCALING else None for r in roles]
    cnt = getattr(self, "send_to_gpui_cnt", None)
    if cnt is not None:
        srcs.append(cnt)
        keys.append(("send_to_gpui_cnt", None))
        roles.append(dgr.DENSIFY_ROLE_COPY)
        alts.append(None)
    srcs = [t.detach().contiguous() for t in srcs]
    dsts = [arena.destination(key, t, n_new) for key, t in zip(keys, srcs)]
    dgr.densify_move(cls, ranks, (n_orig, n_clone, n_child, n_split), srcs, dsts, roles, alts,
                     self._rotation.detach().contiguous(), samples, copies=N)
    views = [d[:n_new] for d in dsts]
    _replace_optimizer_rows(self, slots, views[:len(slots)])
    if cnt is not None:
        self.send_to_gpui_cnt = views[-1]
    for key, v in zip(keys, views):
        arena.release_other(key, v)
    self.xyz_gradient_accum = arena.zeros("xyz_gradient_accum", n_new, (1,))
    self.denom = arena.zeros("denom", n_new, (1,))
    self.max_radii2D = arena.zeros("max_radii2D", n_new)
    self.sum_visible_count_in_one_batch = arena.zeros("sum_visible_count_in_one_batch", n_new)
    arena.events += 1


# --------------------------------------------------------------------------------- redistribution
def redistribute_rows(tensors, destination, group):
    """send row i of every tensor to rank destination[i]: ONE packed all-to-all-v.  Returns the received
    tensors (rows ordered by source rank, original order inside a source) and the i->j size matrix."""
    W = group.size()
    order, counts = dgr.group_rows(destination, W)
    n_send = sum(counts[:W])
    widths = [math.prod(t.shape[1:]) for t in tensors]
    R = sum(widths)
    dev = tensors[0].device
    send = torch.empty((n_send, R), dtype=torch.float32, device=dev)
    cols, c = [], 0
    for w in widths:
        cols.append((c, c + w))
        c += w
    # int32 tensors travel bit-exactly as 4-byte words of the fp32 record
    srcs = [t.view(torch.float32) if t.dtype != torch.float32 else t for t in tensors]
    srcs = [s.reshape(s.shape[0], -1) for s in srcs]
    dgr.gather_rows(order, n_send, srcs, [send[:, a:b] for a, b in cols])
    local = torch.tensor(counts[:W], dtype=torch.int32, device=dev)
    i2j = torch.empty((W * W,), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(i2j, local, group=group)
    i2j = i2j.view(W, W).cpu().tolist()
    rank = group.rank()
    recv_splits = [i2j[i][rank] for i in range(W)]
    recv = torch.empty((sum(recv_splits), R), dtype=torch.float32, device=dev)
    dist.all_to_all_single(recv, send, output_split_sizes=recv_splits, input_split_sizes=counts[:W], group=group)
    n_new = recv.shape[0]
    outs = [torch.empty((n_new,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in tensors]
    dgr.gather_rows(None, n_new, [recv[:, a:b] for a, b in cols], [o.reshape(n_new, -1) for o in outs])
    outs = [o.view(t.dtype) if t.dtype != torch.float32 else o for o, t in zip(outs, tensors)]
    return outs, i2j


def need_redistribute_gaussians(self, group):
    """scene/gaussian_model.py:1245-1262"""
    args = utils.get_args()
    if group.size() == 1:
        return False
    if utils.get_denfify_iter() == args.redistribute_gaussians_frequency:
        return True
    all_n = [None for _ in range(group.size())]
    dist.all_gather_object(all_n, self._xyz.shape[0], group=group)
    return min(all_n) * args.redistribute_gaussians_threshold < max(all_n)


def redistribute_gaussians(self, destination=None, group=None):
    """random rebalancing of the shards (scene/gaussian_model.py:1264-1329); `destination` / `group` default to
    the reference's choices (uniform random destination, the default group)"""
    args = utils.get_args()
    if getattr(args, "redistribute_gaussians_mode", "random_redistribute") == "no_redistribute":
        return
    group = group if group is not None else utils.DEFAULT_GROUP
    if destination is None:
        if not need_redistribute_gaussians(self, group):
            return
        if args.redistribute_gaussians_mode != "random_redistribute":
            raise ValueError("Invalid redistribute_gaussians_mode: " + args.redistribute_gaussians_mode)
        destination = torch.randint(0, group.size(), (self._xyz.shape[0],), device=self._xyz.device)
    slots = _optimizer_slots(self)
    outs, _ = redistribute_rows([_slot_tensor(self, g, k) for g, k in slots], destination, group)
    _replace_optimizer_rows(self, slots, outs)
    n, dev = self._xyz.shape[0], self._xyz.device
    self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    self.denom = torch.zeros((n, 1), device=dev)
    self.max_radii2D = torch.zeros((n,), device=dev)
    self.sum_visible_count_in_one_batch = torch.zeros((n,), device=dev)
    self.send_to_gpui_cnt = torch.zeros((n, group.size()), dtype=torch.int, device=dev)


# ----------------------------------------------------------------------- statistics / opacity reset
def add_densification_stats(self, viewspace_point_tensor, update_filter, absgrad=None):
    """scene/gaussian_model.py:1046-1052: accumulate |d loss / d means2D| (the op's NDC-scaled gradient) of the
    Gaussians visible in this view.  Same values as the reference's `x[filter] += norm(grad[filter, :2])` for ANY filter,
    without its boolean indexing (a `nonzero` host sync + gather + scatter per statement): the rows outside the filter
    receive + 0.
    `absgrad` (extension of this build, see update_densification_stats): a [P,2] tensor whose norm is accumulated
    instead of the signed gradient's; `viewspace_point_tensor.grad` is then not read."""
    f = update_filter.view(-1, 1)
    g = viewspace_point_tensor.grad if absgrad is None else absgrad
    n = torch.linalg.vector_norm(g[:, :2], dim=-1, keepdim=True)
    self.xyz_gradient_accum += torch.where(f, n, torch.zeros((), dtype=n.dtype, device=n.device))
    self.denom += f


def update_densification_stats(self, viewspace_point_tensor, radii, absgrad=None):
    """What densification.py:13-25 of the reference does after every backward of the densification phase -- for the
    visible Gaussians (radii > 0): max_radii2D = max(max_radii2D, radii), then add_densification_stats -- WITHOUT the
    boolean indexing (two `nonzero` host syncs and six gather / scatter kernels per camera and iteration: measured 0.54 ms
    of a 1.18 ms step at 10^6 Gaussians).  The mask is implied by the data: an invisible Gaussian has radius 0 (the maximum
    leaves max_radii2D alone, radii are never negative) and a means2D gradient of exactly 0 (K10 never touches its row
    of the zero-initialised record; the mirror exchange scatter-adds into zeros), so the unmasked updates change the
    same rows by the same amounts, bit for bit; `denom` counts the rows with radius > 0.
    `absgrad` (extension of this build; None: everything above, bit for bit): the camera's [P,2] absolute screen-space
    gradient (gaussian_renderer.set_absgrad / collect_absgrad; include/gsraster.h: gsr_render_absgrad) -- its norm
    replaces the signed gradient's norm in xyz_gradient_accum, `viewspace_point_tensor.grad` is not read, max_radii2D
    and denom are as before.  The sum of magnitudes is at least the magnitude of the sum, and several times larger on
    the large Gaussians it is meant to find, so `densify_grad_threshold` NEEDS RETUNING under it (gsplat's default
    goes from 0.0002 to 0.0008 with absgrad); this project fixes no value."""
    if absgrad is not None and (absgrad.dim() != 2 or absgrad.shape[0] != radii.shape[0] or absgrad.shape[1] < 2):
        raise ValueError("update_densification_stats: `absgrad` must be [P, 2] with one row per entry of `radii`")
    g = viewspace_point_tensor.grad if absgrad is None else absgrad
    if (radii.dtype == torch.int32 and g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1 and
            all(t.dtype == torch.float32 and t.is_contiguous() for t in (self.max_radii2D, self.xyz_gradient_accum,
                                                                         self.denom))):
        dgr.densify_stats(radii, g, self.max_radii2D, self.xyz_gradient_accum, self.denom)  # ONE launch
        return
    r = radii if radii.dtype == torch.float32 else radii.float()
    torch.maximum(self.max_radii2D, r.view_as(self.max_radii2D), out=self.max_radii2D)
    self.xyz_gradient_accum += torch.linalg.vector_norm(g[:, :2], dim=-1, keepdim=True)
    self.denom += (radii > 0).view_as(self.denom)


def replace_tensor_to_optimizer(self, tensor, name):
    """scene/gaussian_model.py:770-791: swap one parameter for a new tensor, zeroing its Adam moments"""
    out = {}
    for group in self.optimizer.param_groups:
        if group["name"] != name:
            continue
        old = group["params"][0]
        st = self.optimizer.state.get(old, None)
        if st is not None:
            for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
                if key in st:
                    st[key] = torch.zeros_like(tensor)
            del self.optimizer.state[old]
        group["params"][0] = nn.Parameter(tensor.requires_grad_(True))
        if st is not None:
            self.optimizer.state[group["params"][0]] = st
        out[name] = group["params"][0]
    return out


def reset_opacity(self):
    """scene/gaussian_model.py:555-561: opacity <- min(opacity, 0.01), in logit space"""
    _log("Resetting opacity to 0.01\n")
    o = torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01)
    new = torch.log(o / (1 - o))
    self._opacity = replace_tensor_to_optimizer(self, new, "opacity")["opacity"]


def prune_by_contribution(self, scores, min_wmax=None, min_hits=1):
    """Prune the rows no training view made use of (no counterpart in the reference): `scores` is the
    diff_gaussian_rasterization.ContributionStats that gaussian_renderer.score_contributions accumulated over the views,
    one row per local Gaussian.  A row goes when fewer than `min_hits` pixels blended it or, with `min_wmax`, when its
    largest blend weight on any pixel stayed below that (RadSplat's rule).  The thresholds are absolute, so the ranks
    need no agreement.  -> the number of rows pruned"""
    if not isinstance(scores, dgr.ContributionStats) or scores.P != self._xyz.shape[0]:
        raise ValueError("prune_by_contribution: `scores` must be a ContributionStats with one row per local Gaussian")
    mask = scores.hits < int(min_hits)
    if min_wmax is not None:
        mask = torch.logical_or(mask, scores.wmax < float(min_wmax))
    n = int(mask.sum())
    _log("Number of gaussians pruned by contribution: {}\n".format(n))
    if n:
        prune_points(self, mask)
    return n


def install(cls):
    """graft level B3: make these functions the methods of the reference's GaussianModel class"""
    for fn in (prune_points, prune_by_contribution, cat_tensors_to_optimizer, densification_postfix, densify_and_clone, densify_and_split,
               densify_and_prune, densify_and_prune_fused, need_redistribute_gaussians, redistribute_gaussians,
               add_densification_stats, update_densification_stats,
               replace_tensor_to_optimizer, reset_opacity):
        setattr(cls, fn.__name__, fn)
    return cls
