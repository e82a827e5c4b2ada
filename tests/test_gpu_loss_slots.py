"""csrc/loss.hip where its passes are cut: rows around the 32-row tile and the 42-row halo, widths around the four-column
tasks of the horizontal pass and the 16-byte staging vectors.

The forward keeps its x y map a scalar chain (the compiler is stopped from pairing adjacent outputs of it) and adds its
two sums through one pair of barriers; each output's tap chain and each sum's order are what they were.  Shapes: 3 channels x rows in {1, 5, 31, 32, 33, 43} x W in {4, 8, 36, 44, 45} (45: the scalar staging),
and a device band whose first row is not a multiple of 32.  Checks, with test_gpu_loss_edges' launcher (guard bands
around every buffer, NaN rows around the band) and its bounds:
  * the three maps, the image gradient for both coefficient sets and the two sums against leaf_refs.loss_reference in
    float64 (helpers.assert_elem_close, K = 8 times the float32 reference's own error; the sums by SUM_FLOOR);
  * bitwise where leaf_refs.loss_kernel_order_fp32 has the kernel's bits: the restatement multiplies and adds where the
    kernel contracts to fma, and divides where the kernel takes v_rcp_f32, so that is the L1 part of the gradient
    (a launch with g_ssim = 0: gl1 * sign(x - y), formed as the restatement forms it);
  * the device-band launch bit-equal to the static one (same tiles, same chains)."""
import pytest
import torch

import leaf_refs as R
import test_gpu_loss_edges as E

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 31, 32, 33, 43]
WIDTHS = [4, 8, 36, 44, 45]
L1_ONLY = [(0.7, 0.0, 0.8 / 7.0, 1.0)]


def _l1_part_bitwise(device, c, x, gt, y0, y1, cap, tag):
    got = E.run_loss(device, c["img"], c["gt"], y0, y1, cap=cap, coefs=L1_ONLY)["grads"][0]
    f = torch.float32
    d = x[:, y0:y1].to(f) - gt[:, y0:y1].to(f) * torch.tensor(1.0 / 255.0, dtype=f)
    sgn = (d > 0).to(f) - (d < 0).to(f)
    want = torch.tensor(L1_ONLY[0][0], dtype=f) * torch.tensor(L1_ONLY[0][2], dtype=f) * sgn
    # (loss_kernel_order_fp32's own first term, gl1 * sgn, for these coefficients; its SSIM term is times an exact zero)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{tag}: L1 part of the gradient differs in bits"


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_loss_rows_and_widths(device, rows, W):
    C, y0, y1 = 3, 0, rows
    c = E._case("noise", C, rows, W, y0, y1)
    tag = f"noise {C}x{rows}x{W}"
    static = E.run_loss(device, c["img"], c["gt"], y0, y1)
    E._check_against_fp64(static, c, tag + " static")
    dyn = E.run_loss(device, c["img"], c["gt"], y0, y1, cap=rows + 7)
    E._check_against_fp64(dyn, c, tag + f" cap{rows + 7}")
    E._bit_equal(dyn, static, tag + " device band vs static")
    x, gt, _ = R.loss_inputs("noise", C, rows, W)
    _l1_part_bitwise(device, c, x, gt, y0, y1, None, tag)


@pytest.mark.parametrize("family", ["noise", "ties"])
@pytest.mark.parametrize("W", [44, 45])
def test_loss_device_band_off_the_tile_grid(device, family, W):
    """rows [27, 70) of a 96-row image: the band's first row is not a multiple of 32, 43 rows = one tile and 11 rows"""
    C, H, y0, y1 = 3, 96, 27, 70
    c = E._case(family, C, H, W, y0, y1)
    tag = f"{family} {C}x{H}x{W}[{y0}:{y1}]"
    static = E.run_loss(device, c["img"], c["gt"], y0, y1)
    E._check_against_fp64(static, c, tag + " static")
    for cap in (y1 - y0, 96):
        dyn = E.run_loss(device, c["img"], c["gt"], y0, y1, cap=cap)
        E._check_against_fp64(dyn, c, tag + f" cap{cap}")
        E._bit_equal(dyn, static, tag + f" cap{cap} vs static")
    x, gt, _ = R.loss_inputs(family, C, H, W)
    _l1_part_bitwise(device, c, x, gt, y0, y1, 96, tag)
