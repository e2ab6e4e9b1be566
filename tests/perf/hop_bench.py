"""Decimated output against the route it replaces, on one GPU, alternated in one process, at config 2 (N = 2^20, 256 scales,
fp64 Morlet(6), tau = 1e-9) for hop in {256, 1024}:

  A. the engine alone (device events on the plan's stream): cwt_transform_hop with the power output against
     cwt_transform_power followed by P[:, ::h].contiguous() on the device;
  B. cwt_power_device(hop=h) against cwt_power_device followed by [:, ::h] on the device (host clock around calls that end in a
     synchronise: upload of the signal, allocation, transform);
  C. cwt_power_torch(hop=h) forward + backward against cwt_power_torch + slice, forward + backward (device events);
  D. the two hop kernels alone (option "profile": every kernel class bracketed by events), for "hop_fuse_terms" in
     {0, 1, 2, 4, 16, all}: 0 = every row through hop_fold and scratch, all = every row folded inside hop_rows.

Each comparison: warm-up of both routes, then `--reps` rounds of (old, new), medians and the spread.  Not collected by pytest.
Usage: python tests/perf/hop_bench.py [--hops 256,1024] [--reps 20] [--out profiles/hop_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, ROWS, TAU = 1 << 20, 256, 1e-9


def scale_grid(flambda):
    s0 = 2 / flambda
    return s0, np.log2(N / s0) / (ROWS - 1), s0 * 2 ** (np.arange(ROWS) * np.log2(N / s0) / (ROWS - 1))


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(torch, old, new, reps, clock):
    for _ in range(3):
        old()
        new()
    torch.cuda.synchronize()
    to, tn = [], []
    for _ in range(reps):
        to.append(clock(torch, old))
        tn.append(clock(torch, new))
    to, tn = np.array(to), np.array(tn)
    return ("old %8.3f ms (min %.3f max %.3f)   hop %8.3f ms (min %.3f max %.3f)   old/hop %.1f" %
            (np.median(to), to.min(), to.max(), np.median(tn), tn.min(), tn.max(), np.median(to) / np.median(tn)))


class DevicePointer:
    """a device buffer of a DevicePower as a torch tensor (zero copy)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", default="256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hop_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("hop_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    m = pycwt_amd.Morlet(6)
    s0, dj, sj = scale_grid(m.flambda())
    dev = torch.device("cuda:0")
    xn = np.random.default_rng(1234).standard_normal(N)
    x = torch.from_numpy(xn).to(dev)
    lines = ["Decimated power output against cwt_transform_power + slice: N = 2^20, 256 scales, fp64 Morlet(6), tau = 1e-9, %s, build %s."
             % (torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max).  Written by tests/perf/hop_bench.py." % args.reps, ""]
    pycwt_amd.set_tolerance(TAU)
    for hop in [int(h) for h in args.hops.split(",")]:
        nch = N // hop
        lines.append("hop = %d (M = %d, output %d x %d reals = %.1f MB against %.1f MB)" % (hop, nch, ROWS, nch, ROWS * nch * 8 / 1e6, ROWS * N * 8 / 1e6))
        # A. the engine alone
        plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
        plan.set_stream(torch.cuda.current_stream().cuda_stream)
        P = torch.empty((ROWS, N), dtype=torch.float64, device=dev)
        Ph = torch.empty((ROWS, nch), dtype=torch.float64, device=dev)
        keep = []

        def old_engine():
            plan.transform_power(x.data_ptr(), N, 0, 6.0, 1.0, sj, None, P.data_ptr(), N, N)
            keep[:] = [P[:, ::hop].contiguous()]

        def new_engine():
            plan.transform_hop(x.data_ptr(), 1, N, N, 0, 6.0, 1.0, sj, hop, None, 1, Ph.data_ptr(), nch)
        lines.append("  A engine, power        " + alternate(torch, old_engine, new_engine, args.reps, event_ms))
        ref = keep[0]
        err = ((Ph - ref).abs().amax(dim=1) / P.amax(dim=1)).max().item()
        lines.append("    hop output against the slice of the existing output (tau = 1e-9): per-row max |dP| / max P = %.2e" % err)
        # D. the hop kernels alone, per fuse threshold
        plan.set_option("profile", 1)
        for fuse in (0, 1, 2, 4, 16, 65536):
            plan.set_option("hop_fuse_terms", fuse)
            for _ in range(3):
                new_engine()
            plan.timings()
            for _ in range(args.reps):
                new_engine()
            t = plan.timings()
            per = {k: v[0] / args.reps * 1e3 for k, v in t.items()}          # (timings() resets the plan's accumulators: cwt_hip.h)
            hop_us = sum(v for k, v in per.items() if k.startswith("hop_"))
            lines.append("  D hop_fuse_terms %-6s " % ("all" if fuse == 65536 else fuse) +
                         "   ".join("%s %.1f us" % (k, per[k]) for k in sorted(per)) + "   fold + inverse %.1f us" % hop_us)
        plan.close()
        del P, Ph, ref, keep
        # B. the Python functions that keep the result on the device
        def old_device():
            r = pycwt_amd.cwt_power_device(xn, 1.0, dj, s0, ROWS - 1, m)
            full = torch.as_tensor(DevicePointer(r.device_ptr, (ROWS, N), "<f8"), device=dev)
            out = full[:, ::hop].contiguous()
            torch.cuda.synchronize()
            r.close()
            return out

        def new_device():
            pycwt_amd.cwt_power_device(xn, 1.0, dj, s0, ROWS - 1, m, hop=hop).close()
        lines.append("  B cwt_power_device     " + alternate(torch, old_device, new_device, max(5, args.reps // 2), wall_ms))
        # C. torch, forward + backward
        gPh = torch.randn((ROWS, nch), dtype=torch.float64, device=dev)

        def old_torch():
            xa = x.clone().requires_grad_(True)
            (pycwt_amd.cwt_power_torch(xa, 1.0, dj, s0, ROWS - 1, m)[0][:, ::hop] * gPh).sum().backward()

        def new_torch():
            xa = x.clone().requires_grad_(True)
            (pycwt_amd.cwt_power_torch(xa, 1.0, dj, s0, ROWS - 1, m, hop=hop)[0] * gPh).sum().backward()
        lines.append("  C cwt_power_torch f+b  " + alternate(torch, old_torch, new_torch, max(5, args.reps // 2), event_ms))
        lines.append("")
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
