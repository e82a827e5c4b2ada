"""Shared helpers of the parity tests: seeded scenes, camera kwargs, error metrics."""
import math

import torch

import synthetic_scene as S
from oracle import cref as C
from oracle import torch_oracle as O

KEYS = ["means3D", "scales", "rotations", "shs", "opacities"]


def cam_kwargs(cam, sh_degree=3, device="cpu"):
    return dict(viewmatrix=cam.world_view_transform.to(device), projmatrix=cam.full_proj_transform.to(device),
                campos=cam.camera_center.to(device), W=cam.image_width, H=cam.image_height,
                tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), sh_degree=sh_degree)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def frac_bad(a, b, rtol=1e-3, atol=1e-5):
    """fraction of elements outside |a-b| <= atol + rtol*|b| (threshold flips show up here)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    bad = (a - b).abs() > (atol + rtol * b.abs())
    return bad.double().mean().item()


def elem_excess(a, b, rtol=1e-4, atol_rms=1e-5, q=0.99):
    """element-wise tolerance test of SURVEY.md 8(c)'s fidelity ladder ("norm-wise AND p99 element-wise"):
    the q-quantile over the non-zero reference entries of |a-b| / (rtol*|b| + atol), atol = atol_rms * rms(b).
    <= 1 means: at least a fraction q of the entries satisfy |a-b| <= rtol*|b| + atol.
    Measured fp32-noise bound (oracle/gsraster_ref.c in fp32 against the fp64 autograd oracle, same scenes):
    p99 <= 0.30, p99.9 <= 0.92 for every gradient tensor with atol_rms = 1e-5 -- so a HIP result that passes
    with value <= 1 is inside ~3x the rounding noise of a plain fp32 CPU implementation."""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    nz = b != 0
    if int(nz.sum()) == 0:
        return float((a - b).abs().max()) if a.numel() else 0.0
    rms = b[nz].pow(2).mean().sqrt()
    ratio = (a - b).abs()[nz] / (rtol * b[nz].abs() + atol_rms * rms)
    if ratio.numel() > 2_000_000:  # torch.quantile input limit: subsample deterministically
        ratio = ratio[:: ratio.numel() // 2_000_000 + 1]
    return float(torch.quantile(ratio, q))


def settings_from(cam, bg, sh_degree=3, device="cuda"):
    from diff_gaussian_rasterization import GaussianRasterizationSettings

    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx / 2),
        tanfovy=math.tan(cam.FoVy / 2), bg=bg.to(device), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(device), projmatrix=cam.full_proj_transform.to(device),
        sh_degree=sh_degree, campos=cam.camera_center.to(device), prefiltered=False, debug=False)


def oracle_c_chain(g, cam, bg, mask, wgt, sh_degree=3):
    """full fwd+bwd through the C restatement; returns dict of everything"""
    kw = cam_kwargs(cam, sh_degree)
    W, H = cam.image_width, cam.image_height
    m2, rgb, co, radii, depths, cov3D, clamped = C.preprocess_forward(*[g[k] for k in KEYS], **kw)
    pl, ranges, tt = C.bin_and_sort(m2, radii, depths, mask, W, H)
    img, fT, nc = C.render_forward(m2, co, rgb, mask, bg, W, H, pl, ranges)
    d2, dco, drgb = C.render_backward(m2, co, rgb, mask, bg, W, H, pl, ranges, fT, nc, wgt)
    dm, ds, dr, dsh, do = C.preprocess_backward(g["means3D"], g["scales"], g["rotations"], g["shs"], radii, cov3D,
                                                clamped, d2, dco, drgb, **kw)
    return dict(means2D=m2, rgb=rgb, conic_opacity=co, radii=radii, depths=depths, cov3D=cov3D, clamped=clamped,
                point_list=pl, ranges=ranges, image=img, final_T=fT, n_contrib=nc, d_means2D=d2, d_conic_opacity=dco,
                d_rgb=drgb, d_means3D=dm, d_scales=ds, d_rotations=dr, d_shs=dsh, d_opacities=do)


# ---------------------------------------------------------------------------- frozen rasterizer goldens
GOLDEN_DIR = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden")
GOLDEN_SCENES = ["single", "two_overlap", "rand10k_256", "behind_camera", "low_opacity", "saturating", "border_band0",
                 "border_band1", "sh0", "sh1", "sh2", "sh3", "white_bg", "black_bg", "rows1080"]


def golden_weight(H, W):
    """dL/dimage of the golden scenes (analytic, float64) -- the same formula as tests/golden/make_raster_golden.py"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    return torch.stack([0.5 + 0.5 * torch.sin(0.37 * x + 0.91 * y + 1.3 * c) for c in range(3)])


def load_golden(name):
    """-> dict(g = the five input tensors (float32), kw = camera kwargs of the oracles, bg, mask (bool [gy,gx]), W, H,
    sh_degree, out = dict of the frozen float64-oracle results (float32 / int32 tensors))"""
    import numpy as np

    z = np.load(__import__("os").path.join(GOLDEN_DIR, f"raster_{name}.npz"))
    W, H, deg = int(z["W"]), int(z["H"]), int(z["sh_degree"])
    if "regen" in z.files:
        n, w, h, seed = [int(v) for v in z["regen"]]
        g = S.make_gaussians(n, w, h, seed=seed, scale_coef=float(z["regen_scale_coef"]))
    else:
        g = {k: torch.from_numpy(z["in_" + k]) for k in KEYS}
    chk = torch.tensor([float(g[k].double().sum()) for k in KEYS] + [float(g[k].double().abs().sum()) for k in KEYS],
                       dtype=torch.float64)
    want = torch.from_numpy(z["input_checksum"])
    assert torch.allclose(chk, want, rtol=1e-12, atol=1e-12), f"golden {name}: inputs are not the frozen ones"
    kw = dict(viewmatrix=torch.from_numpy(z["viewmatrix"]), projmatrix=torch.from_numpy(z["projmatrix"]),
              campos=torch.from_numpy(z["campos"]), W=W, H=H, tanfovx=float(z["tanfovx"]), tanfovy=float(z["tanfovy"]),
              sh_degree=deg)
    out = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out_")}
    return dict(name=name, g=g, kw=kw, bg=torch.from_numpy(z["bg"]), mask=torch.from_numpy(z["mask"]), W=W, H=H,
                sh_degree=deg, out=out)


def c_chain_kw(g, kw, bg, mask, wgt):
    """oracle_c_chain for explicit camera kwargs (the goldens carry matrices, not camera objects)"""
    W, H = kw["W"], kw["H"]
    m2, rgb, co, radii, depths, cov3D, clamped = C.preprocess_forward(*[g[k] for k in KEYS], **kw)
    pl, ranges, tt = C.bin_and_sort(m2, radii, depths, mask, W, H)
    img, fT, nc = C.render_forward(m2, co, rgb, mask, bg, W, H, pl, ranges)
    d2, dco, drgb = C.render_backward(m2, co, rgb, mask, bg, W, H, pl, ranges, fT, nc, wgt)
    dm, ds, dr, dsh, do = C.preprocess_backward(g["means3D"], g["scales"], g["rotations"], g["shs"], radii, cov3D,
                                                clamped, d2, dco, drgb, **kw)
    return dict(means2D=m2, rgb=rgb, conic_opacity=co, radii=radii, depths=depths, image=img, final_T=fT, n_contrib=nc,
                d_means2D=d2, d_conic_opacity=dco, d_rgb=drgb, d_means3D=dm, d_scales=ds, d_rotations=dr, d_shs=dsh,
                d_opacities=do)


GOLDEN_GRADS = ["d_means2D", "d_means3D", "d_scales", "d_rotations", "d_shs", "d_opacities"]


# ---------------------------------------------------------------------------- element-wise check against fp64
def elem_tolerance(ref64, ref32, K=8):
    """K * max(max|ref32 - ref64|, 4 * 2^-24 * max|ref64|): the reference's own fp32 error (the same reference code run
    in float32 on the CPU), never the kernel's, with a floor of four half-ulps of the largest value"""
    r64, r32 = ref64.detach().double().cpu(), ref32.detach().double().cpu()
    if r64.numel() == 0:
        return 0.0
    e32 = float((r32 - r64).abs().max())
    floor = 4.0 * 2.0 ** -24 * float(r64.abs().max())
    return K * max(e32, floor)


def assert_elem_close(got, ref64, ref32, K=8, what=""):
    """every element: |got - ref64| <= K * max(max|ref32 - ref64|, floor) (elem_tolerance); no element is excluded, a
    NaN fails.  -> the observed ratio max|got - ref64| / max(max|ref32 - ref64|, floor), for the caller's log"""
    g, r64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r64.shape, f"{what}: shape {tuple(g.shape)} != {tuple(r64.shape)}"
    if r64.numel() == 0:
        return 0.0
    tol = elem_tolerance(ref64, ref32, K)
    unit = tol / K
    err = (g - r64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    worst = int(err.reshape(-1).argmax())
    ratio = float(err.reshape(-1)[worst]) / unit if unit > 0 else (0.0 if float(err.max()) == 0 else float("inf"))
    if not ratio <= K:
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), err.shape)) if err.dim() else ()
        raise AssertionError(f"{what}: element {idx}: got {g.reshape(-1)[worst].item():.9g}, fp64 reference "
                             f"{r64.reshape(-1)[worst].item():.9g}, error / unit = {ratio:.3g} > K = {K} "
                             f"(unit = {unit:.3g})")
    return ratio


# ---------------------------------------------------------------------------- row-wise check against fp64
ROW_UNIT_FLOOR = 4.0 * 2.0 ** -24    # four half-ulps of the row's largest value
ROW_UNIT_CAP = 4096.0 * 2.0 ** -24   # 2.4e-4: a case whose reference is worse conditioned than this gets other inputs


def rows_unit(ref64, ref32):
    """the worst per-row relative error of a plain fp32 implementation on these inputs: max(ROW_UNIT_FLOOR, max over the
    rows with s_i > 0 of e32_i / s_i), s_i = max_c |ref64[i,c]|, e32_i = max_c |ref32[i,c] - ref64[i,c]|.  ref32 is the
    same reference code run in float32 on the CPU, never the kernel's result."""
    r64, r32 = ref64.detach().double().cpu(), ref32.detach().double().cpu()
    assert r64.shape == r32.shape, f"shape {tuple(r64.shape)} != {tuple(r32.shape)}"
    if r64.numel() == 0:
        return ROW_UNIT_FLOOR
    r64, r32 = r64.reshape(r64.shape[0], -1), r32.reshape(r32.shape[0], -1)
    s = r64.abs().amax(dim=1)
    e32 = (r32 - r64).abs().amax(dim=1)
    assert not bool(torch.isnan(s).any() | torch.isnan(e32).any()), "NaN in the reference"
    live = s > 0
    worst = float((e32[live] / s[live]).max()) if bool(live.any()) else 0.0
    return max(ROW_UNIT_FLOOR, worst)


def assert_rows_close(got, ref64, ref32, K=8, what=""):
    """every row i of [N, ...] tensors (flattened to [N, C]), nothing excluded:
        max_c |got[i,c] - ref64[i,c]| <= K * unit * s_i,   s_i = max_c |ref64[i,c]|,   unit = rows_unit(ref64, ref32);
    a row with s_i == 0 must be exactly zero in `got`; a NaN fails.  unit <= ROW_UNIT_CAP is asserted before `got` is
    looked at (a cap on the case's conditioning, not a measurement).  -> (unit, worst err_i / (unit * s_i))"""
    unit = rows_unit(ref64, ref32)
    assert unit <= ROW_UNIT_CAP, (f"{what}: the fp32 reference is off by {unit / 2.0 ** -24:.0f} x 2^-24 of a row's largest "
                                  f"value, over the cap of {ROW_UNIT_CAP / 2.0 ** -24:.0f}: change the inputs of this case")
    g, r64 = got.detach().double().cpu(), ref64.detach().double().cpu()
    assert g.shape == r64.shape, f"{what}: shape {tuple(g.shape)} != {tuple(r64.shape)}"
    if r64.numel() == 0:
        return unit, 0.0
    g, r64 = g.reshape(g.shape[0], -1), r64.reshape(r64.shape[0], -1)
    s = r64.abs().amax(dim=1, keepdim=True)
    err = (g - r64).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    # ratio per element; on a zero row any non-zero (or NaN) entry is infinitely far off
    ratio = torch.where(s > 0, err / (unit * s.clamp(min=1e-300)),
                        torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = int(ratio.reshape(-1).argmax())
    i, c = divmod(worst, ratio.shape[1])
    w = float(ratio[i, c])
    if not w <= K:
        raise AssertionError(f"{what}: row {i}, column {c}: got {float(g[i, c]):.9g}, fp64 reference "
                             f"{float(r64[i, c]):.9g}, error / (unit * row max) = {w:.3g} > K = {K} "
                             f"(unit = {unit:.3g}, row max = {float(s[i, 0]):.3g})")
    return unit, w
