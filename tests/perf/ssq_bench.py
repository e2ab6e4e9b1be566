"""The steps of the synchrosqueezed transform on one GPU, alternated in one process, at config 2 (N = 2^20, 256 scales, fp64
Morlet(6), tau = 1e-9), for two signals: white noise -- the worst case for the reassignment: the instantaneous frequency of
neighbouring rows jumps, so the cell held in registers changes with almost every entry -- and a unit chirp in noise of std 0.01
(a ridge: the rows around it share a bin):

  transform      (a) cwt_transform: W
  derivative     (b) cwt_spectrum_derivative + cwt_transform_rows: dW
  reassign       (c) cwt_ssq_reassign with accumulate = 0 (zero-fill of T + the reassignment), gamma = sqrt(eps) std, the default grid
  c, no fill         the same with accumulate = 1: no zero-fill
  c, one cell        accumulate = 1, a grid of ONE bin that takes every entry: the log2, no cell traffic
  c, all dropped     accumulate = 1, gamma = 1e300: every entry dropped at the first test -- the read stream alone
  icwt           cwt_reduce_scales over the same W (k_icwt): the read-rate yardstick, half the bytes of (c)

Device events on the plan's stream around each step; 3 warm-up rounds, then `--reps` rounds of all steps in turn; medians and the
spread, and the rate over the bytes each step must read (W and dW: 2 x rows x N x 16 B; icwt: half).  Then the per-kernel-class times
(option "profile").  There is no pass mark: the numbers are a record.  Not collected by pytest.
Usage: python tests/perf/ssq_bench.py [--reps 20] [--out profiles/ssq_bench.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssq_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("ssq_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    rng = np.random.default_rng(1234)
    t = np.arange(N)
    signals = (("white noise", rng.standard_normal(N)),
               ("chirp 0.001 ... 0.2 cycles per sample + noise of std 0.01",
                np.cos(2 * np.pi * (0.001 * t + 0.5 * (0.199 / N) * t * t)) + 0.01 * rng.standard_normal(N)))
    text = "\n".join(run(torch, pycwt_amd, _hip, lib, args.reps, name, xs) for name, xs in signals)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def run(torch, pycwt_amd, _hip, lib, reps, signal, xs):
    mother = pycwt_amd.Morlet(6)
    sj = scale_grid(mother.flambda())
    freqs = 1 / (mother.flambda() * sj)
    dv = float(np.log2(freqs.max() / freqs.min()) / (ROWS - 1))
    f_lo, nf = float(freqs.min()), ROWS
    dev = torch.device("cuda:0")
    gamma = float(np.sqrt(np.finfo(np.float64).eps) * xs.std())
    x = torch.from_numpy(xs).to(dev)
    plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    xh, yh = (torch.empty(N, dtype=torch.complex128, device=dev) for _ in range(2))
    W, dW, T = (torch.empty((ROWS, N), dtype=torch.complex128, device=dev) for _ in range(3))
    out = torch.empty(N, dtype=torch.float64, device=dev)
    w = 1 / np.sqrt(sj)

    def reassign(accumulate, g=gamma, grid=(f_lo, dv, nf)):
        plan.ssq_reassign(W.data_ptr(), dW.data_ptr(), N, N, w, g, grid[0], grid[1], grid[2], T.data_ptr(), N, accumulate)

    def derivative():
        plan.spectrum_derivative(xh.data_ptr(), 1.0, yh.data_ptr())
        plan.transform_rows(yh.data_ptr(), 0, 6.0, 1.0, sj, dW.data_ptr(), N, N)
    steps = (("transform", lambda: plan.transform(x.data_ptr(), N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N), 0),
             ("derivative", derivative, 0),
             ("reassign", lambda: reassign(False), 2),
             ("c, no fill", lambda: reassign(True), 2),
             ("c, one cell", lambda: reassign(True, grid=(1e-30, 400.0, 1)), 2),
             ("c, all dropped", lambda: reassign(True, g=1e300), 2),
             ("icwt", lambda: plan.reduce_scales(W.data_ptr(), N, N, w, False, 1.0, out.data_ptr()), 1))
    for _ in range(3):
        for _, fn, _ in steps:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in steps}
    for _ in range(reps):
        for name, fn, _ in steps:
            times[name].append(event_ms(torch, fn))
    reassign(False)
    torch.cuda.synchronize()
    kept = float((T != 0).sum().item()) / T.numel()
    lines = ["Steps of the synchrosqueezed transform: N = 2^20, 256 scales, fp64 Morlet(6), tau = 1e-9, %s, %d bins, %s, build %s."
             % (signal, nf, torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max) of device events; rate = the bytes the step "
             "must read (W, or W and dW) over the median.  Written by tests/perf/ssq_bench.py." % reps, ""]
    matrix = ROWS * N * 16
    for name, _, reads in steps:
        t = np.array(times[name])
        rate = "   %.2f TB/s" % (reads * matrix / (np.median(t) * 1e-3) / 1e12) if reads else ""
        lines.append("%-15s %8.3f ms (min %.3f max %.3f)%s" % (name, np.median(t), t.min(), t.max(), rate))
    med = {name: float(np.median(times[name])) for name, _, _ in steps}
    lines += ["", "zero-fill %.3f ms, log2 %.3f ms, cell traffic %.3f ms of the %.3f ms of (c); non-empty cells of T: %.1f %%; read rate of (c) / read "
              "rate of icwt = %.2f" % (med["reassign"] - med["c, no fill"], med["c, one cell"] - med["c, all dropped"],
                                       med["c, no fill"] - med["c, one cell"], med["reassign"], 100 * kept,
                                       2 * med["icwt"] / med["reassign"])]
    plan.set_option("profile", 1)                                   # per kernel class, every kernel alone on the stream
    for name, fn, _ in steps[:3] + steps[-1:]:
        for _ in range(3):
            fn()
        plan.timings()
        for _ in range(reps):
            fn()
        per = {k: v[0] / reps * 1e3 for k, v in plan.timings().items()}
        lines.append("per kernel class, %-10s (profile: serialised, sum %.0f us): " % (name, sum(per.values())) +
                     "  ".join("%s %.1f us" % (k, per[k]) for k in sorted(per)))
    plan.close()
    del W, dW, T
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()
