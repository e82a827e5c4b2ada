"""bench.py --dump-outputs: what a step's caller receives, bounded in size and sampled with fixed seeds."""
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _model(n, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"xyz": (3,), "features_dc": (1, 3), "features_rest": (15, 3), "opacity": (1,), "scaling": (3,),
              "rotation": (4,)}
    return types.SimpleNamespace(**{"_" + k: torch.randn(n, *s, generator=g) for k, s in shapes.items()})


def test_dump_outputs_are_bounded_and_reproducible(tmp_path):
    bench = _bench()
    model = _model(bench.DUMP_ROWS + 1000, 0)
    images = [torch.rand(3, 1080, 1920, generator=torch.Generator().manual_seed(k)) for k in range(2)] + [None]
    state = {"loss": torch.tensor(0.25), "images": images}
    a = bench.collect_outputs(model, state)
    b = bench.collect_outputs(model, state)
    assert sorted(a) == ["features_dc", "features_rest", "images", "loss", "opacity", "rotation", "scaling", "xyz"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["loss"].tolist() == [0.25]
    assert a["images"].shape == (bench.DUMP_IMAGE_ELEMS,)  # 3 cameras of 1080p: a seeded sample
    assert a["xyz"].shape == (bench.DUMP_ROWS, 3) and a["features_rest"].shape == (bench.DUMP_ROWS, 15, 3)
    # the sampled rows are rows of the model, in ascending order
    rows = [int(np.nonzero((model._xyz.numpy() == r).all(1))[0][0]) for r in a["xyz"][:50]]
    assert rows == sorted(rows)
    bench.write_outputs(a, str(tmp_path / "out"))
    assert np.array_equal(np.load(str(tmp_path / "out" / "opacity.npy")), a["opacity"])


def test_small_outputs_are_dumped_whole():
    bench = _bench()
    model = _model(500, 1)
    img = torch.rand(3, 96, 160)
    a = bench.collect_outputs(model, {"loss": torch.tensor(1.5), "images": [img]})
    assert a["images"].shape == (1, 3, 96, 160) and np.array_equal(a["images"][0], img.numpy())
    assert np.array_equal(a["rotation"], model._rotation.numpy())


def test_guarded_legs_do_not_dump():
    """the hipGraph leg of a multi-GPU --full run is a child launch with the parent's arguments: without the dump's"""
    bench = _bench()
    argv = ["--gpus", "2", "--dump-outputs", "d", "--full", "--dump-outputs=e", "--steps", "3"]
    assert bench.without_dump(argv) == ["--gpus", "2", "--full", "--steps", "3"]


def test_plain_run_defaults_leave_out_the_full_legs():
    import argparse

    bench = _bench()

    def ns(**kw):
        d = dict(full=False, repeats=None, render_steps=None, no_extra=False, no_cpu_baseline=False, no_legs=False,
                 no_1gpu_leg=False)
        d.update(kw)
        return bench.resolve_run(argparse.Namespace(**d))

    a = ns()
    assert (a.repeats, a.render_steps) == (1, 0)
    assert a.no_extra and a.no_cpu_baseline and a.no_legs and a.no_1gpu_leg
    f = ns(full=True)
    assert (f.repeats, f.render_steps) == (5, 20)
    assert not (f.no_extra or f.no_cpu_baseline or f.no_legs or f.no_1gpu_leg)
    e = ns(repeats=3, render_steps=4)  # explicit values hold in a plain run
    assert (e.repeats, e.render_steps) == (3, 4) and e.no_extra
