"""The total-variation kernel of csrc/bilagrid.hip (include/gsraster.h, N1g: gsr_bilagrid_tv) against fp64 autograd of
tests/bilagrid_refs.tv_reference: the value and every element of the ACCUMULATED gradient, tolerance
helpers.assert_elem_close with the fp32 run of the same reference as the unit."""
import pytest
import torch

import bilagrid_refs as B
from helpers import assert_elem_close

pytestmark = pytest.mark.gpu

K = 8
f32, f64, i32 = torch.float32, torch.float64, torch.int32
CASES = [(3, (3, 5, 4)), (2, B.DEFAULT)]
WEIGHT = 10.0


def _inputs(N, sizes):
    gw, gh, gl = sizes
    g = torch.Generator().manual_seed(17 * N + gw)
    grids = torch.stack([B.make_grid(sizes, 50 + n) for n in range(N)])
    before = torch.randn(N, 12, gl, gh, gw, generator=g)  # what the buffer holds: the kernel adds to it
    return grids, before


def _reference(grids, before, dtype):
    G = grids.to(dtype).clone().requires_grad_(True)
    T = B.tv_reference(G)
    (grad,) = torch.autograd.grad(T, G)
    return T.detach(), before.to(dtype) + dtype_weight(dtype) * grad


def dtype_weight(dtype):
    return torch.tensor(WEIGHT, dtype=dtype)


@pytest.mark.parametrize("N,sizes", CASES)
def test_value_and_accumulated_gradient_against_fp64(device, N, sizes):
    from diff_gaussian_rasterization import bilagrid_tv

    grids, before = _inputs(N, sizes)
    (T64, g64), (T32, g32) = _reference(grids, before, f64), _reference(grids, before, f32)
    buf = before.to(device).clone()
    grad, T = bilagrid_tv(grids.to(device), WEIGHT, grad=buf, value=True)
    assert grad.data_ptr() == buf.data_ptr() and T.shape == ()
    ratio = assert_elem_close(grad.cpu(), g64, g32, K=K, what=f"tv gradient N={N} {sizes}")
    print(f"RATIO bilagrid tv_grad N={N} {sizes} {ratio:.4g}")
    ratio = assert_elem_close(T.cpu().reshape(1), T64.reshape(1), T32.reshape(1), K=K, what=f"tv value N={N} {sizes}")
    print(f"RATIO bilagrid tv_value N={N} {sizes} {ratio:.4g}")
    # without the value: the same gradient bits, in one launch; a fresh buffer starts from zero
    buf2 = before.to(device).clone()
    assert bilagrid_tv(grids.to(device), WEIGHT, grad=buf2) is buf2
    assert torch.equal(buf2.view(i32), grad.view(i32))
    fresh = bilagrid_tv(grids.to(device), WEIGHT)
    only = _reference(grids, torch.zeros_like(before), f64)[1], _reference(grids, torch.zeros_like(before), f32)[1]
    assert_elem_close(fresh.cpu(), only[0], only[1], K=K, what="tv gradient into a fresh buffer")
    # equal grids have no variation: nothing is added, the value is zero
    flat = torch.stack([B.identity_grid(sizes)] * N).to(device)
    buf3 = before.to(device).clone()
    _, T0 = bilagrid_tv(flat, WEIGHT, grad=buf3, value=True)
    assert float(T0) == 0.0 and torch.equal(buf3.cpu(), before)


def test_refused_arguments(device):
    from diff_gaussian_rasterization import bilagrid_tv

    grids = torch.stack([B.make_grid((3, 5, 4), 1)]).to(device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid_tv(grids.cpu(), 1.0)
    with pytest.raises(ValueError):
        bilagrid_tv(grids[0], 1.0)
    with pytest.raises(ValueError):
        bilagrid_tv(grids, 1.0, grad=torch.zeros(1, 12, 4, 5, 2, device=device))
