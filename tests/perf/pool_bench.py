"""The time-pooled scalogram against the routes it replaces, on one GPU, alternated in one process, at config 2 (N = 2^20, 256
scales, fp64 Morlet(6), tau = 1e-9) for pool in {16, 256, 4096}:

  pooled   cwt_transform_pool (the polynomial rows sum their windows in pool_poly_rows, the others go through plan scratch and
           pool_rows);
  power    cwt_transform_power alone (what the pooled step must beat to be worth having: it writes rows x n0 reals);
  power+avg  cwt_transform_power followed by torch.nn.functional.avg_pool1d on the device (the only route before this mode).

Device events on the plan's stream around each step; warm-up of all three, then `--reps` rounds of (pooled, power, power+avg);
medians and the spread.  Then the per-kernel times of one pooled step (option "profile": every kernel class bracketed by events,
side streams off), pool_poly_rows and pool_rows among them, and of one power step for comparison.  There is no pass mark: the
numbers are a record.  Not collected by pytest.
Usage: python tests/perf/pool_bench.py [--pools 16,256,4096] [--reps 20] [--out profiles/pool_bench.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, ROWS, TAU = 1 << 20, 256, 1e-9


def scale_grid(flambda):
    s0 = 2 / flambda
    return s0 * 2 ** (np.arange(ROWS) * np.log2(N / s0) / (ROWS - 1))


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(name, t):
    t = np.array(t)
    return "%-10s %8.3f ms (min %.3f max %.3f)" % (name, np.median(t), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pools", default="16,256,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("pool_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    sj = scale_grid(pycwt_amd.Morlet(6).flambda())
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.random.default_rng(1234).standard_normal(N)).to(dev)
    lines = ["Pooled scalogram against cwt_transform_power and cwt_transform_power + avg_pool1d: N = 2^20, 256 scales, fp64 Morlet(6), "
             "tau = 1e-9, %s, build %s." % (torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max) of device events.  Written by "
             "tests/perf/pool_bench.py." % args.reps, ""]
    plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    P = torch.empty((ROWS, N), dtype=torch.float64, device=dev)
    keep = []

    def power():
        plan.transform_power(x.data_ptr(), N, 0, 6.0, 1.0, sj, None, P.data_ptr(), N, N)
    for pool in [int(h) for h in args.pools.split(",")]:
        nc = N // pool
        Pb = torch.empty((ROWS, nc), dtype=torch.float64, device=dev)

        def pooled():
            plan.transform_pool(x.data_ptr(), 1, N, N, 0, 6.0, 1.0, sj, pool, None, Pb.data_ptr(), nc)

        def power_avg():
            power()
            keep[:] = [torch.nn.functional.avg_pool1d(P[None], pool)[0]]
        steps = (("pooled", pooled), ("power", power), ("power+avg", power_avg))
        for _ in range(3):
            for _, fn in steps:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in steps}
        for _ in range(args.reps):
            for name, fn in steps:
                times[name].append(event_ms(torch, fn))
        err = ((Pb - keep[0]).abs().amax(dim=1) / keep[0].amax(dim=1)).max().item()
        split = plan.last_split()
        lines.append("pool = %d (output %d x %d reals = %.1f MB against %.1f MB; %d of %d rows of polynomial form)"
                     % (pool, ROWS, nc, ROWS * nc * 8 / 1e6, ROWS * N * 8 / 1e6, split["poly"], ROWS))
        lines += ["  " + summary(name, times[name]) for name, _ in steps]
        med = {name: float(np.median(times[name])) for name, _ in steps}
        lines.append("  power / pooled %.2f   power+avg / pooled %.2f   pooled against avg_pool1d of the power: per-row max |d| / max = %.2e"
                     % (med["power"] / med["pooled"], med["power+avg"] / med["pooled"], err))
        plan.set_option("profile", 1)                                   # per kernel class, every kernel alone on the stream
        for name, fn in (("pooled", pooled), ("power", power)):
            for _ in range(3):
                fn()
            plan.timings()
            for _ in range(args.reps):
                fn()
            per = {k: v[0] / args.reps * 1e3 for k, v in plan.timings().items()}
            lines.append("  per kernel class, %-6s (profile: serialised, sum %.0f us): " % (name, sum(per.values())) +
                         "  ".join("%s %.1f us" % (k, per[k]) for k in sorted(per)))
        plan.set_option("profile", 0)
        lines.append("")
        del Pb
        keep.clear()
    plan.close()
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
