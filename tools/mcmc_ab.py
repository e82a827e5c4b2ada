"""3DGS-MCMC cost A/B at ROWS rows (default 10^6):
  * the per-step noise launch (mcmc_noise, xi drawn in the kernel): HIP-event time of blocks of launches, as a fraction
    of the HBM peak for its 56 B / row (44 read + 12 written);
  * one relocate-and-grow event at the cap with 5 % of the rows dead, next to one one-pass clone / split / prune event
    (densification_ops.densify_and_prune_fused, untouched by the MCMC code) on a model of the same size -- the two
    alternate, event by event, each on a freshly prepared model, timed on the host around a device synchronise.
python tools/mcmc_ab.py [ROWS [EVENTS [OUT.txt]]]   (default output: profiles/mcmc_ab.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "grendel-gs_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from densify_event_ab import Model, dev, event  # noqa: E402  (tools/: the model and the timed clone/split/prune event)
from mcmc import MCMCStrategy  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, as bench.py


def kill(m, fraction, seed):
    """`fraction` of the rows die (opacity logit -8: 3e-4), chosen by a seeded draw on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    dead = torch.rand(m._xyz.shape[0], device=dev, generator=g) < fraction
    with torch.no_grad():
        m._opacity.masked_fill_(dead.view(-1, 1), -8.0)


def mcmc_event(st, m, it):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st.relocate_and_grow(m, it)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    events = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "mcmc_ab.txt")
    import utils.general_utils as utils
    utils.GLOBAL_RANK, utils.WORLD_SIZE = 0, 1
    utils.DEFAULT_GROUP = utils.IN_NODE_GROUP = utils.SingleGPUGroup()
    utils.set_args(utils.default_args(bsz=1))
    lines = [f"tools/mcmc_ab.py {n} {events} on {torch.cuda.get_device_name(0)} (torch {torch.__version__})"]

    # ---- the noise launch
    a = Model(n, 1)
    st = MCMCStrategy(cap_max=n, seed=1)
    for it in range(20):  # warm-up: code object load, clocks
        st.inject_noise(a, it, 1.6e-4)
    block, blocks = 200, 7
    per = []
    for b in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for it in range(block):
            st.inject_noise(a, 1000 + b * block + it, 1.6e-4)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / block)
    med = statistics.median(per)
    gbs = 56.0 * n / (med * 1e-3) / 1e9
    lines.append(f"noise launch, {n} rows, {blocks} blocks of {block} back-to-back launches (HIP events): median "
                 f"{med * 1e3:.1f} us per launch (min {min(per) * 1e3:.1f}, max {max(per) * 1e3:.1f}); 56 B/row -> "
                 f"{gbs:.0f} GB/s = {gbs / HBM_PEAK_GBS:.3f} of the {HBM_PEAK_GBS:.0f} GB/s HBM peak "
                 "(the working set fits the 256 MiB Infinity Cache at 10^6 rows: a rate above HBM's is a cache rate)")
    del a

    # ---- the events, alternating
    mc, fu, rows_f = [], [], []
    m = Model(n, 2)
    st = MCMCStrategy(cap_max=n, seed=2)
    kill(m, 0.05, 0)
    mcmc_event(st, m, 0)  # warm-up (at the cap nothing is copied into the arena: rows are relocated where they are)
    for ev in range(events):
        kill(m, 0.05, 100 + ev)
        mc.append(mcmc_event(st, m, 1 + ev))
        b = Model(n, 3 + ev)
        kill(b, 0.05, 100 + ev)
        torch.manual_seed(ev)
        fu.append(event(b, True))
        rows_f.append(int(b._xyz.shape[0]))
        del b
        print(ev, round(mc[-1], 3), round(fu[-1], 3), rows_f[-1], flush=True)
    assert m._xyz.shape[0] == n
    lines.append(f"relocate-and-grow event at the cap ({n} rows, 5 % dead, host clock around a synchronise), {events} "
                 f"events alternating with the one-pass event: median {statistics.median(mc):.3f} ms "
                 f"(min {min(mc):.3f}, max {max(mc):.3f}); rows after every event: {n}")
    lines.append(f"one-pass clone/split/prune event (densify_and_prune_fused, 2 % of the rows over the gradient threshold, "
                 f"same 5 % dead; a fresh model and arena per event, so its first-event allocations are included): median "
                 f"{statistics.median(fu):.3f} ms (min {min(fu):.3f}, max {max(fu):.3f}); rows after: "
                 f"{min(rows_f)}..{max(rows_f)}")
    # the one-pass event once more on a model whose arena is warm (second event of the same model)
    b = Model(n, 50)
    kill(b, 0.05, 7)
    event(b, True)
    b.fresh(51)
    kill(b, 0.05, 8)
    warm = event(b, True)
    lines.append(f"one-pass event, second event of one model (arena warm): {warm:.3f} ms at {int(b._xyz.shape[0])} rows")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
