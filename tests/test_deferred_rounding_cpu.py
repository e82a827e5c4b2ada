"""CPU: the host-side rules of deferred rounding (diff_gaussian_rasterization: _DEFERRED) -- when a render backward may
leave the rounding of K10's record to the fused K11 + Adam launch, the pointer-identity rule by which the projection
backward decides between handing on sums and flags and rounding first, and the lazy `.grad` view.  No kernel runs: the
records' materialize() is a stand-in that counts (the launches themselves: tests/test_gpu_k11_sums.py,
tests/test_gpu_deferred_rounding.py)."""
import types

import pytest
import torch

import diff_gaussian_rasterization as dgr

P = 6


class FakeSink:
    fuse_backward, sparse = True, False

    def __init__(self, accept=True):
        self.accept, self.offered = accept, []

    def accepts(self, params):
        return self.accept

    def offer(self, pending):
        self.offered.append(pending)


class CountingRecord(dgr._DeferredRecord):
    """a deferred record on the host whose rounding is a copy"""

    def __init__(self):
        acc = torch.arange(P * 9, dtype=torch.float64).view(P, 9) + 0.5
        super().__init__(torch.full((P, 9), float("nan")), acc, torch.ones(P, dtype=torch.uint8), None)
        self.calls = 0

    def materialize(self):
        if not self.materialized:
            self.materialized = True
            self.calls += 1
            self.record.copy_(self.acc64.float())


@pytest.fixture(autouse=True)
def _clean():
    yield
    dgr.set_deferred_backward_sink(None)
    dgr.set_deferred_rounding("env")
    dgr._DEFERRED.clear()
    dgr._CAPTURE[0] = None


def test_switch_and_arming_conditions():
    armed = {"_gsr_defer_record": True}
    dgr.set_deferred_rounding("env")
    assert dgr.deferred_rounding() is True  # on unless GSR_DEFER_ROUNDING=0
    assert not dgr._defer_armed(armed, 100, True)  # no sink
    sink = FakeSink()
    dgr.set_deferred_backward_sink(sink)
    assert dgr._defer_armed(armed, 100, True)
    assert not dgr._defer_armed({}, 100, True) and not dgr._defer_armed(None, 100, True)  # the caller did not ask
    assert not dgr._defer_armed(armed, 100, False)  # no row flags (GSR_TOUCHED_ROWS=0)
    assert not dgr._defer_armed(armed, 1, True)     # a one-row gradient is passed on as a dense copy
    dgr.set_deferred_rounding(False)
    assert dgr.deferred_rounding() is False and not dgr._defer_armed(armed, 100, True)
    dgr.set_deferred_rounding(True)
    assert dgr._defer_armed(armed, 100, True)
    sink.sparse = True  # the sparse update classifies the rows from the record
    assert not dgr._defer_armed(armed, 100, True)
    sink.sparse, sink.fuse_backward = False, False
    assert not dgr._defer_armed(armed, 100, True)
    sink.fuse_backward = True
    dgr._CAPTURE[0] = object()  # a hipGraph capture keeps today's launches
    assert not dgr._defer_armed(armed, 100, True)
    dgr._CAPTURE[0] = None
    with pytest.raises(ValueError):
        dgr.set_deferred_rounding("sometimes")


def test_pointer_identity_rule():
    e = CountingRecord()
    r = e.record
    assert e.is_view(r[:, 0:2], 0, 2) and e.is_view(r[:, 2:5], 2, 3) and e.is_view(r[:, 5:9], 5, 4)
    assert not e.is_view(r[:, 2:5].clone(), 2, 3)          # equal values elsewhere
    assert not e.is_view(r[:, 0:2], 2, 2)                  # another column block
    assert not e.is_view(r[:, 0:3], 0, 2)                  # another width
    assert not e.is_view(r[:-1, 0:2], 0, 2)                # fewer rows
    other = torch.zeros((P, 18))
    assert not e.is_view(other[:, 0:2], 0, 2)              # another buffer, another stride
    assert not e.is_view(None, 0, 2)


def _node(B, entries_at=None, needs_cam_grad=False):
    """a stand-in ctx of _PreprocessGaussiansRawBatched on the host, and its saved tensors"""
    params = (torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 4), torch.zeros(P, 1, 3), torch.zeros(P, 15, 3),
              torch.zeros(P, 1))
    m2 = torch.zeros(B, P, 2)
    ctx = types.SimpleNamespace(
        saved_tensors=params + (torch.zeros(B, 40), torch.ones(B, P, dtype=torch.int32), torch.zeros(P, 6),
                                torch.zeros(B, P, 3, dtype=torch.uint8)),
        meta=(3, 1.0, 64, 48, 16, False), m2_ptr=m2.data_ptr(), tanfov0=(0.5, 0.5), cuda_args_list=None,
        needs_input_grad=(True,) * 6 + (needs_cam_grad,) + (False,) * 6)
    return ctx, m2


def _grads(entries, edit=None):
    g = []
    for k, e in enumerate(entries):
        r = e.record
        g += [r[:, 0:2], r[:, 2:5], r[:, 5:9], None, None]
    if edit is not None:
        g[edit[0]] = edit[1]
    return g


@pytest.mark.parametrize("B", [1, 2])
def test_projection_backward_hands_on_sums_only_for_the_records_own_views(B):
    back = dgr._PreprocessGaussiansRawBatched.backward
    sink = FakeSink()
    dgr.set_deferred_backward_sink(sink)

    def fresh(file_under_key=True):
        ctx, m2 = _node(B)
        entries = [CountingRecord() for _ in range(B)]
        for k, e in enumerate(entries):
            dgr._register_deferred(m2[k].data_ptr() if file_under_key else 1000 + k, e)
        return ctx, m2, entries

    # every gradient IS its record's view: sums and flags go on, nothing is rounded
    ctx, m2, entries = fresh()
    out = back(ctx, *_grads(entries))
    assert all(o is None for o in out) and len(sink.offered) == 1
    pend = sink.offered.pop()
    assert pend.deferred == entries and sum(e.calls for e in entries) == 0 and not dgr._DEFERRED
    if B == 1:  # the views travel too, lazily: a reader that takes them instead of the sums has the record rounded
        assert pend.gstride == 9 and type(pend.g_means2D) is dgr._LazyRecordView and entries[0].calls == 0
    pend.round_records()  # (what materialize() and the sparse launch do first)
    assert pend.deferred is None and all(e.calls == 1 for e in entries)
    want = torch.stack([e.acc64.float() for e in entries])
    assert torch.equal(pend.g_means2D.reshape(B, P, 2), want[:, :, 0:2])
    assert torch.equal(pend.g_rgb.reshape(B, P, 3), want[:, :, 2:5])
    assert torch.equal(pend.g_conic_opacity.reshape(B, P, 4), want[:, :, 5:9])

    # the record is found through the gradient's address when means2D reached the render op as a copy
    ctx, m2, entries = fresh(file_under_key=False)
    back(ctx, *_grads(entries))
    assert sink.offered.pop().deferred == entries and not dgr._DEFERRED

    # a gradient that never arrived (an unused output): rounded first, then the record path
    ctx, m2, entries = fresh()
    back(ctx, *_grads(entries, edit=(1, None)))
    pend = sink.offered.pop()
    assert pend.deferred is None and all(e.calls == 1 for e in entries)

    # the switch went off between the render backward and this node
    ctx, m2, entries = fresh()
    dgr.set_deferred_rounding(False)
    back(ctx, *_grads(entries))
    dgr.set_deferred_rounding(True)
    assert sink.offered.pop().deferred is None and all(e.calls == 1 for e in entries)

    # a sparse sink reads the record
    ctx, m2, entries = fresh()
    sink.sparse = True
    back(ctx, *_grads(entries))
    sink.sparse = False
    assert sink.offered.pop().deferred is None and all(e.calls == 1 for e in entries)

    # a tensor that is not the view: autograd has added something to unrounded memory -- refuse loudly
    ctx, m2, entries = fresh()
    with pytest.raises(RuntimeError, match="set_deferred_rounding"):
        back(ctx, *_grads(entries, edit=(0, entries[0].record[:, 0:2] + 1.0)))


def test_lazy_view_rounds_on_first_use_and_not_before():
    e = CountingRecord()
    dgr._register_deferred(1, e)
    g = e.record[:, 0:2]
    v = dgr.lazy_record_view(g)
    assert type(v) is dgr._LazyRecordView
    x = torch.zeros(P, 2)
    x.grad = v                       # keeping it reads nothing
    assert x.grad is not None and e.calls == 0
    n = torch.linalg.vector_norm(x.grad[:, :2], dim=-1)
    assert e.calls == 1 and type(n) is torch.Tensor
    assert torch.equal(n, torch.linalg.vector_norm(e.acc64.float()[:, :2], dim=-1))
    assert x.grad.data_ptr() == g.data_ptr() and e.calls == 1  # once
    # a rounded record, or a tensor outside every pending record, is passed through as it is
    assert dgr.lazy_record_view(g) is g
    t = torch.zeros(3, 2)
    assert dgr.lazy_record_view(t) is t and dgr.lazy_record_view(None) is None
    # the address alone is a use too (a launch takes it)
    e2 = CountingRecord()
    dgr._register_deferred(2, e2)
    v2 = dgr.lazy_record_view(e2.record[:, 0:2])
    v2.data_ptr()
    assert e2.calls == 1


def test_lazy_view_is_found_in_keyword_and_nested_arguments():
    def lazy():
        e = CountingRecord()
        dgr._register_deferred(id(e), e)
        return e, dgr.lazy_record_view(e.record[:, 0:2])

    e, v = lazy()
    got = torch.add(torch.ones(P, 2), other=v)  # a keyword argument
    assert e.calls == 1 and torch.equal(got, e.acc64.float()[:, 0:2] + 1.0)
    e, v = lazy()
    got = torch.cat(tensors=[torch.zeros(1, 2), v])
    assert e.calls == 1 and torch.equal(got[1:], e.acc64.float()[:, 0:2])
    e, v = lazy()
    got = torch.block_diag(*[v])  # (positional, for comparison)
    assert e.calls == 1
    e, v = lazy()
    out = torch.empty(P, 2)
    torch.mul(torch.ones(P, 2), 2.0, out=out)
    torch.add(out, v, out=out)
    assert e.calls == 1 and torch.equal(out, e.acc64.float()[:, 0:2] + 2.0)


def test_a_record_that_leaves_the_bounded_table_is_rounded():
    entries = [CountingRecord() for _ in range(40)]
    for k, e in enumerate(entries):
        dgr._register_deferred(k, e)
    assert len(dgr._DEFERRED) == dgr._DEFERRED_MAX and 39 in dgr._DEFERRED
    gone = [e for k, e in enumerate(entries) if k not in dgr._DEFERRED]
    assert len(gone) == 40 - dgr._DEFERRED_MAX and all(e.calls == 1 for e in gone)
    assert all(torch.equal(e.record, e.acc64.float()) for e in gone)
    assert all(e.calls == 0 for e in dgr._DEFERRED.values())


def test_more_views_than_the_table_holds_all_come_out_rounded():
    """a batch of 20 views whose render backwards all file their records before the ONE projection backward runs (a
    caller that armed them all; the mirror does not arm a batch of more than DEFER_MAX_CAMERAS): the first four leave
    the table rounded, the projection backward rounds the rest, and the record path gets every view's gradient"""
    B = 20
    assert B > dgr._DEFERRED_MAX > dgr.DEFER_MAX_CAMERAS
    sink = FakeSink()
    dgr.set_deferred_backward_sink(sink)
    ctx, m2 = _node(B)
    entries = [CountingRecord() for _ in range(B)]
    for k, e in enumerate(entries):
        e.acc64 += 100.0 * k  # (every view its own values)
        dgr._register_deferred(m2[k].data_ptr(), e)
    dgr._PreprocessGaussiansRawBatched.backward(ctx, *_grads(entries))
    pend = sink.offered.pop()
    assert pend.deferred is None and all(e.calls == 1 for e in entries) and not dgr._DEFERRED
    want = torch.stack([e.acc64.float() for e in entries])
    assert torch.equal(pend.g_means2D.reshape(B, P, 2), want[:, :, 0:2])
    assert torch.equal(pend.g_rgb.reshape(B, P, 3), want[:, :, 2:5])
    assert torch.equal(pend.g_conic_opacity.reshape(B, P, 4), want[:, :, 5:9])
    # nine views, all found: more than one sums launch takes, so they are rounded and take the record path as well
    ctx, m2 = _node(9)
    entries = [CountingRecord() for _ in range(9)]
    for k, e in enumerate(entries):
        dgr._register_deferred(m2[k].data_ptr(), e)
    dgr._PreprocessGaussiansRawBatched.backward(ctx, *_grads(entries))
    assert sink.offered.pop().deferred is None and all(e.calls == 1 for e in entries)
