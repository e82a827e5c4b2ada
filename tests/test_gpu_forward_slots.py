"""K8's slots through the C ABI: where in a 64-entry chunk the relevant entries sit.

gsr_render_forward / gsr_render_backward on the cases of tests/forward_slot_cases.py (and the short `lengths` cases of
composite_refs, whose last group holds 1, 2 or 3 entries): the list position n_contrib takes comes from the pair record,
and the slots behind a chunk's last relevant entry are inert records, so the cases put relevant and irrelevant entries
side by side, the last blended entry on chunk index 0, 63 and 64, every residue of the four-slot groups in front of and
behind a full chunk, an opacity of exactly 0 among live ones, and partial tiles.  `n_contrib` equals the float64
reference on every pixel; image, final_T and the four gradient groups of the backward (which must take the forward's
decisions) meet helpers.assert_rows_close with composite_refs' K.  Every case runs without and with the segment
workspace (the two SEG instantiations of K8): with it the forward is bit-equal, the backward meets the same rule.

`test_slab_poisoned_by_the_preceding_launch` runs each case right behind a launch of the same lists whose colours are
1e30, with outputs pre-filled with NaN: a slot that picked up what the earlier launch left in LDS shows as a wrong
pixel (colours of that size times any weight) or a NaN."""
import pytest
import torch

import composite_refs as R
import forward_slot_cases as S
import test_gpu_composite_pixels as P

pytestmark = pytest.mark.gpu

CASES = tuple(c for c in R.cases() if c.family == "lengths" and c.name in ("1", "2", "3", "5", "7", "9")) + S.cases()
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_backward_against_float64(device, case):
    fwd, rec = P._root(case, device)
    fig = P._check_forward(case, fwd, case.id)
    fig.update(P._check_record(case, rec, case.id))
    P._print("slots", case, fig)


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
    P._print("slots-segments", case, P._check_record(case, rec, f"{case.id} segments"))


class _Poison(P._Dev):
    """the case's lists and geometry with colours of 1e30"""

    def __init__(self, d):
        self.__dict__.update(d.__dict__)
        self.rgb = torch.full_like(d.rgb, 1e30)


@pytest.mark.parametrize("seg", [False, True], ids=["plain", "segments"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_slab_poisoned_by_the_preceding_launch(device, case, seg):
    root, _ = P._root(case, device)
    d = P._dev(case, device)
    ws = P._seg_ws(case, device) if seg else None
    assert P._forward(_Poison(d), seg=ws)[0] == 0
    fwd = P._forward(d, seg=ws)
    assert fwd[0] == 0
    P._assert_forward_bits(fwd, root, f"{case.id} behind a launch with colours of 1e30")
    P._check_forward(case, fwd, f"{case.id} poisoned")
