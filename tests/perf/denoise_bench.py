"""The steps of wavelet shrinkage on one GPU, alternated in one process, at config 2 (N = 2^20, 256 scales, fp64 Morlet(6),
tau = 1e-9), white noise:

  transform      cwt_transform: W (for scale; not part of the comparison)
  select         cwt_row_order_statistics of |W|^2, the two middle ranks of every row (the median of an even count)
  shrink <mode>  cwt_icwt_shrink with the universal thresholds of those medians, on the device
  icwt           cwt_icwt_reduce over the same W (k_icwt): the read-rate yardstick of the shrink-inverse
  torch ...      the same steps as torch operations on the device: kthvalue of |W| (both ranks), the soft rule element-wise, sum
  denoise        the whole pycwt_amd.denoise call from a host array to host arrays (a host clock around it: uploads, the transform,
                 allocation of W, the selection, the shrink-inverse, downloads)

Device events on the plan's stream around each step; 3 warm-up rounds, then `--reps` rounds of all steps in turn; medians and the
spread, and the rate over the bytes each step must read (W = rows x N x 16 B; the selection: that times the reads it takes).  The
number of reads of the selection is computed from the data by the kernel's own rule (11-bit digits of the key of the rank's value,
counting rounds until at most 2048 candidates share the prefix, plus the compaction read) and shown beside its time in units of
the icwt read.  Then the per-kernel-class times (option "profile").  There is no pass mark: the numbers are a record.  Not
collected by pytest.
Usage: python tests/perf/denoise_bench.py [--reps 20] [--out profiles/denoise_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, ROWS, TAU = 1 << 20, 256, 1e-9
DIGIT, CAP = 11, 2048


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


def reads_by_the_rule(torch, W, ranks, chunk=16):
    """per (row, rank): the counting rounds until at most CAP entries share the leading digits of the rank's key, plus one"""
    out = []
    for r0 in range(0, W.shape[0], chunk):
        v = W[r0:r0 + chunk].real ** 2 + W[r0:r0 + chunk].imag ** 2
        keys = torch.sort(v, dim=1).values.view(torch.int64)              # (positive doubles: their bits order them)
        per_rank = []
        for k in ranks:
            m = keys[:, k:k + 1]
            rounds = torch.full((keys.shape[0],), 64 // DIGIT + 1, dtype=torch.int64, device=W.device)
            for d in range(64 // DIGIT, 0, -1):
                shift = 64 - DIGIT * d
                lo = (m >> shift) << shift
                cand = torch.searchsorted(keys, lo + (1 << shift)) - torch.searchsorted(keys, lo)
                rounds = torch.where(cand[:, 0] <= CAP, torch.full_like(rounds, d), rounds)
            per_rank.append(rounds + 1)
        out.append(torch.stack(per_rank, dim=1))
        del v, keys
    return torch.cat(out).cpu().numpy()                                   # rows x ranks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("denoise_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    reps = args.reps
    mother = pycwt_amd.Morlet(6)
    sj = scale_grid(mother.flambda())
    dev = torch.device("cuda:0")
    xs = np.random.default_rng(1234).standard_normal(N)
    x = torch.from_numpy(xs).to(dev)
    plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    xh = torch.empty(N, dtype=torch.complex128, device=dev)
    W = torch.empty((ROWS, N), dtype=torch.complex128, device=dev)
    stats = torch.empty((ROWS, 2), dtype=torch.float64, device=dev)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    ranks = [N // 2 - 1, N // 2]
    c = float(np.sqrt(np.log(4.0)))
    w_t = torch.from_numpy(1 / np.sqrt(sj)).to(dev)
    plan.transform(x.data_ptr(), N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N)
    plan.row_order_statistics(W.data_ptr(), True, N, N, ROWS, ranks, stats.data_ptr(), 2)
    lam = (0.5 * (stats[:, 0].sqrt() + stats[:, 1].sqrt()) / c * float(np.sqrt(2 * np.log(N)))).contiguous()
    torch.cuda.synchronize()
    torch_out = {}

    def torch_select():
        a = W.abs()
        torch_out["med"] = 0.5 * (torch.kthvalue(a, ranks[0] + 1, dim=1).values + torch.kthvalue(a, ranks[1] + 1, dim=1).values)

    def torch_soft():
        a = W.abs()
        torch_out["y"] = (W.real * torch.clamp(1 - lam[:, None] / a, min=0) * w_t[:, None]).sum(dim=0)

    steps = [("transform", lambda: plan.transform(x.data_ptr(), N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N), 0),
             ("select", lambda: plan.row_order_statistics(W.data_ptr(), True, N, N, ROWS, ranks, stats.data_ptr(), 2), None)]
    steps += [("shrink " + m, lambda m=m: plan.icwt_shrink(W.data_ptr(), N, N, sj, lam.data_ptr(), m, 1.0, out.data_ptr()), 1)
              for m in ("hard", "soft", "garrote")]
    steps += [("icwt", lambda: plan.icwt_reduce(W.data_ptr(), N, N, sj, 1.0, out.data_ptr()), 1),
              ("torch select", torch_select, 0), ("torch soft", torch_soft, 0)]
    for _ in range(3):
        for _, fn, _ in steps:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in steps}
    for _ in range(reps):
        for name, fn, _ in steps:
            times[name].append(event_ms(torch, fn))
    # the same answers from both routes
    med_dev = 0.5 * (stats[:, 0].sqrt() + stats[:, 1].sqrt())
    med_err = float(((med_dev - torch_out["med"]).abs() / torch_out["med"]).max())
    plan.icwt_shrink(W.data_ptr(), N, N, sj, lam.data_ptr(), "soft", 1.0, out.data_ptr())
    torch.cuda.synchronize()
    y_err = float((out - torch_out["y"]).abs().max() / torch_out["y"].abs().max())
    torch_out.clear()
    reads = reads_by_the_rule(torch, W, ranks)
    matrix = ROWS * N * 16
    med = {name: float(np.median(times[name])) for name, _, _ in steps}
    lines = ["Steps of wavelet shrinkage: N = 2^20, 256 scales, fp64 Morlet(6), tau = 1e-9, white noise, %s, build %s."
             % (torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max) of device events; rate = the bytes the step "
             "must read over the median.  Written by tests/perf/denoise_bench.py." % reps, ""]
    for name, _, nread in steps:
        t = np.array(times[name])
        if nread is None:
            nread = float(reads.max(axis=1).mean())      # a row is read until its last rank is done; ranks that share a prefix share the read
        rate = "   %.2f TB/s" % (nread * matrix / (np.median(t) * 1e-3) / 1e12) if nread else ""
        lines.append("%-15s %8.3f ms (min %.3f max %.3f)%s" % (name, np.median(t), t.min(), t.max(), rate))
    lines += ["", "selection: full reads of a row by the kernel's rule (counting rounds + the compaction read), over the %d rows x 2 ranks: "
              "min %d, median %d, max %d, mean over the rows of the larger of the two %.2f; its time = %.2f reads of W at the rate of icwt"
              % (ROWS, reads.min(), np.median(reads), reads.max(), reads.max(axis=1).mean(), med["select"] / med["icwt"]),
              "shrink-inverse rate / icwt rate: " + ", ".join("%s %.2f" % (m, med["icwt"] / med["shrink " + m]) for m in ("hard", "soft", "garrote")),
              "torch route / this route: select %.1f x, soft shrink-inverse %.1f x; the two routes agree: medians to %.1e relative, "
              "y to %.1e of its peak" % (med["torch select"] / med["select"], med["torch soft"] / med["shrink soft"], med_err, y_err)]
    # the whole call, host clock (it ends in downloads: synchronised)
    dj = float(np.log2(N / sj[0]) / (ROWS - 1))
    whole = []
    for i in range(3 + max(3, reps // 4)):
        t0 = time.perf_counter()
        y = pycwt_amd.denoise(xs, 1.0, dj, sj[0], ROWS - 1, mother, precision=64)[0]
        whole.append((time.perf_counter() - t0) * 1e3)
    whole = np.array(whole[3:])
    lines += ["denoise (whole call, host clock, %d calls after 3): %.2f ms (min %.2f max %.2f); y is %s of %d samples"
              % (whole.size, np.median(whole), whole.min(), whole.max(), y.dtype, y.size)]
    plan.set_option("profile", 1)                                   # per kernel class, every kernel alone on the stream
    for name, fn, _ in steps[1:6]:
        for _ in range(3):
            fn()
        plan.timings()
        for _ in range(reps):
            fn()
        per = {k: (v[0] / reps * 1e3, v[1] // reps) for k, v in plan.timings().items()}
        lines.append("per kernel class, %-14s (profile: serialised): " % name +
                     "  ".join("%s %.1f us in %d timed group(s)" % (k, per[k][0], per[k][1]) for k in sorted(per)))
    plan.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
