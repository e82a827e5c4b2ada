"""K10's slots through the C ABI: how many entries of a 64-entry chunk are relevant in a quadrant, and where they sit.

gsr_render_forward / gsr_render_backward on the cases of tests/backward_slot_cases.py.  K10's walk runs on a trip count
of whole pairs: whether a pixel blended an entry and which row of the wave's result table the entry's sums go to both
come from the position word of its pair record, an odd count leaves one inert record behind the last entry, and the
(q, w) rows go through the matrix pipe every eight slots and once more for the rest.  So the cases put every count that
ends a pair, a batch or a chunk differently into quadrant 0, different counts into the four quadrants of one chunk, a
chunk that is all fillers for three quadrants between two that are not, the last blended entry on chunk index 0, 63 and
64, an opacity of exactly 0 among live ones, 130 entries that every pixel takes, and a partial tile.

The record meets helpers.assert_rows_close against float64 with composite_refs' K, without and with the segment
workspace.  `test_lds_poisoned_by_the_preceding_launch` runs each case right behind a backward launch of the same lists
whose colours and pixel gradients are 1e30, with the sums, the record and the row flags cleared by the forward as the
operator has it: an inert slot that picked up what the earlier launch left in LDS shows as a NaN or a huge row, and
`touched` flags exactly the rows that received a non-zero value."""
import pytest
import torch

import backward_slot_cases as B
import composite_refs as R
import test_gpu_composite_pixels as P

pytestmark = pytest.mark.gpu

CASES = B.cases()
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_against_float64(device, case):
    fwd, rec = P._root(case, device)
    fig = P._check_forward(case, fwd, case.id)
    fig.update(P._check_record(case, rec, case.id))
    P._print("bwd-slots", case, fig)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_with_segment_workspace(device, case):
    root, _ = P._root(case, device)
    d = P._dev(case, device)
    seg = P._seg_ws(case, device)
    fwd = P._forward(d, seg=seg)
    assert fwd[0] == 0
    P._assert_forward_bits(fwd, root, f"{case.id} segments")
    code, rec, _ = P._backward(d, fwd, seg=seg)
    assert code == 0
    P._print("bwd-slots-segments", case, P._check_record(case, rec, f"{case.id} segments"))


class _Poison(P._Dev):
    """the case's lists and geometry with colours and pixel gradients of 1e30"""

    def __init__(self, d):
        self.__dict__.update(d.__dict__)
        self.rgb = torch.full_like(d.rgb, 1e30)
        self.g = torch.full_like(d.g, 1e30)


@pytest.mark.parametrize("seg", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lds_poisoned_by_the_preceding_launch(device, case, seg):
    root, root_rec = P._root(case, device)
    d = P._dev(case, device)
    n = case.P
    ws = P._seg_ws(case, device) if seg else None
    buf = torch.full((108 * n + ((n + 15) & ~15),), 0xFF, dtype=torch.uint8, device=device)
    fwd = P._forward(d, seg=ws, zero=buf)  # (clears the sums, the record and the flags; leaves the checkpoints)
    assert fwd[0] == 0
    P._assert_forward_bits(fwd, root, f"{case.id} flagged")
    scratch = torch.zeros_like(buf)
    assert P._backward(_Poison(d), fwd, seg=ws, flagged=scratch)[0] == 0
    code, rec, touched = P._backward(d, fwd, seg=ws, flagged=buf)
    assert code == 0
    what = f"{case.id} behind a backward launch with colours and gradients of 1e30"
    rec = rec.cpu()
    assert bool(torch.isfinite(rec).all()), f"{what}: the record holds a NaN or an inf"
    if not seg:
        assert torch.equal(rec.view(torch.int32), root_rec.cpu().view(torch.int32)), f"{what}: record differs from the root form"
    P._check_record(case, rec, what)
    r64, _ = R.references(case)
    live = torch.cat([r64[k] != 0 for k in R.GROUPS], dim=1).any(dim=1).to(torch.uint8)
    got = touched[:n].cpu()
    assert torch.equal(got, (rec != 0).any(dim=1).to(torch.uint8)), f"{what}: touched differs from the rows that hold a value"
    assert torch.equal(got, live), f"{what}: touched differs on rows {torch.nonzero(got != live).reshape(-1)[:8].tolist()}"
    assert not bool(touched[n:].any())
