"""The steps of the differentiable synchrosqueezed transform on one GPU, alternated in one process, at config 2 (N = 2^20, 256
scales, fp64 Morlet(6), white noise -- the worst case: the bin of neighbouring rows jumps, so the cell held in registers changes
with almost every entry):

  reassign          cwt_ssq_reassign, accumulate = 0 (the yardstick of the next line)
  reassign + bins   cwt_ssq_reassign_bins on the same arguments: the same walk plus one int16 per entry
  gather            cwt_ssq_gather through that map; rate over bins + G + the cells it loads (a cell is loaded when the bin differs
                    from the previous row's of the stretch, counted on the host from the map)
  gather, dropped   the same with a map of -1 everywhere: bins read, zeros written, no cell loaded
  gather, one bin   the same with a map of one bin for all: one cell per stretch of 8 rows
  icwt              cwt_reduce_scales over W (k_icwt): the read-rate yardstick
  ssq_cwt_torch fwd / fwd + bwd, ssq_cwt_device, cwt_torch fwd + bwd: whole calls on the same signal

Device events on torch's current stream around each step; 3 warm-up rounds, then `--reps` rounds of all steps in turn; medians and
the spread.  There is no pass mark: the numbers are a record.  Not collected by pytest.
Usage: python tests/perf/ssq_grad_bench.py [--reps 20] [--out profiles/ssq_grad_bench.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, ROWS, TAU = 1 << 20, 256, 1e-9


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssq_grad_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("ssq_grad_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    dev = torch.device("cuda:0")
    xs = np.random.default_rng(1234).standard_normal(N)
    mother = pycwt_amd.Morlet(6)
    s0 = 2 / mother.flambda()
    dj = float(np.log2(N / s0) / (ROWS - 1))
    sj = s0 * 2 ** (np.arange(ROWS) * dj)
    freqs = 1 / (mother.flambda() * sj)
    f_lo, dv, nf = float(freqs.min()), dj, ROWS
    gamma = float(np.sqrt(np.finfo(np.float64).eps) * xs.std())
    w = 1 / np.sqrt(sj)
    x = torch.from_numpy(xs).to(dev)
    pycwt_amd.set_tolerance(TAU)                               # the shim and the torch entry points at the target of the plan below
    plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    xh = torch.empty(N, dtype=torch.complex128, device=dev)
    W, dW, T, G = (torch.empty((ROWS, N), dtype=torch.complex128, device=dev) for _ in range(4))
    bins = torch.empty((ROWS, N), dtype=torch.int16, device=dev)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    plan.transform(x.data_ptr(), N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N)
    plan.spectrum_derivative(xh.data_ptr(), 1.0, xh.data_ptr())
    plan.transform_rows(xh.data_ptr(), 0, 6.0, 1.0, sj, dW.data_ptr(), N, N)
    plan.ssq_reassign_bins(W.data_ptr(), dW.data_ptr(), N, N, w, gamma, f_lo, dv, nf, T.data_ptr(), N, False, bins.data_ptr(), N)
    torch.cuda.synchronize()
    gT = torch.complex(torch.randn((nf, N), dtype=torch.float64, device=dev), torch.randn((nf, N), dtype=torch.float64, device=dev))
    dropped, one = torch.full_like(bins, -1), torch.full_like(bins, 7)
    # the cells the gather loads: a kept entry whose bin differs from the previous row's, or that is the first kept one of its stretch of 8
    b3 = bins.reshape(ROWS // 8, 8, N)
    kept = b3 >= 0
    loads, cur = 0, torch.full((ROWS // 8, N), -1, dtype=torch.int16, device=dev)
    for u in range(8):
        new = kept[:, u] & (b3[:, u] != cur)
        loads += int(new.sum().item())
        cur = torch.where(kept[:, u], b3[:, u], cur)
    kept_frac = float(kept.float().mean().item())
    del b3, kept, cur, new

    def gather(m):
        plan.ssq_gather(gT.data_ptr(), N, nf, m.data_ptr(), N, w, N, G.data_ptr(), N)
    entries = ROWS * N
    steps = [("reassign", lambda: plan.ssq_reassign(W.data_ptr(), dW.data_ptr(), N, N, w, gamma, f_lo, dv, nf, T.data_ptr(), N, False), 0),
             ("reassign + bins", lambda: plan.ssq_reassign_bins(W.data_ptr(), dW.data_ptr(), N, N, w, gamma, f_lo, dv, nf, T.data_ptr(), N,
                                                                False, bins.data_ptr(), N), 0),
             ("gather", lambda: gather(bins), entries * 18 + loads * 16),
             ("gather, dropped", lambda: gather(dropped), entries * 18),
             ("gather, one bin", lambda: gather(one), entries * 18 + (entries // 8) * 16),
             ("icwt", lambda: plan.reduce_scales(W.data_ptr(), N, N, w, False, 1.0, out.data_ptr()), entries * 16)]
    for _ in range(3):
        for _, fn, _ in steps:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in steps}
    for _ in range(args.reps):
        for name, fn, _ in steps:
            times[name].append(event_ms(torch, fn))
    plan.ssq_reassign_bins(W.data_ptr(), dW.data_ptr(), N, N, w, gamma, f_lo, dv, nf, T.data_ptr(), N, False, bins.data_ptr(), N)
    plan.sync()
    plan.close()
    del W, dW, T, G, gT, dropped, one, bins
    torch.cuda.empty_cache()

    # whole calls
    kw = dict(dj=dj, J=ROWS - 1, wavelet=mother)
    C = None

    def torch_fwd():
        return pycwt_amd.ssq_cwt_torch(x, 1.0, gamma=gamma, **kw)[0]

    def torch_fwd_bwd():
        nonlocal C
        xt = x.clone().requires_grad_(True)
        Tx = pycwt_amd.ssq_cwt_torch(xt, 1.0, gamma=gamma, **kw)[0]
        if C is None:
            C = torch.complex(torch.randn(Tx.shape, dtype=torch.float64, device=dev), torch.randn(Tx.shape, dtype=torch.float64, device=dev))
        Tx.backward(C)
        return xt.grad

    def cwt_fwd_bwd():
        xt = x.clone().requires_grad_(True)
        Wt = pycwt_amd.cwt_torch(xt, 1.0, **kw)[0]
        Wt.backward(C)
        return xt.grad

    def device_call():
        pycwt_amd.ssq_cwt_device(xs, 1.0, gamma=gamma, **kw).close()
    calls = [("ssq_cwt_torch fwd", torch_fwd), ("ssq_cwt_torch fwd + bwd", torch_fwd_bwd), ("cwt_torch fwd + bwd", cwt_fwd_bwd),
             ("ssq_cwt_device (host signal in, T left on the device)", device_call)]
    for _ in range(3):
        for _, fn in calls:
            fn()
    torch.cuda.synchronize()
    ctimes = {name: [] for name, _ in calls}
    for _ in range(args.reps):
        for name, fn in calls:
            ctimes[name].append(event_ms(torch, fn))

    lines = ["Steps of the differentiable synchrosqueezed transform: N = 2^20, 256 scales, fp64 Morlet(6), white noise, %d bins, %s, build %s."
             % (nf, torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max) of device events.  Written by "
             "tests/perf/ssq_grad_bench.py." % args.reps,
             "Kept entries: %.1f %%; cells the gather loads: %.3f per entry (%.2f GB with bins and G)." % (100 * kept_frac, loads / entries,
                                                                                                        (entries * 18 + loads * 16) / 1e9), ""]
    for name, _, nbytes in steps:
        t = np.array(times[name])
        rate = "   %.2f TB/s over %.2f GB" % (nbytes / (np.median(t) * 1e-3) / 1e12, nbytes / 1e9) if nbytes else ""
        lines.append("%-18s %8.3f ms (min %.3f max %.3f)%s" % (name, np.median(t), t.min(), t.max(), rate))
    med = {name: float(np.median(v)) for name, v in times.items()}
    rate = {name: nbytes / med[name] for name, _, nbytes in steps if nbytes}
    lines += ["", "the map costs %.1f %% of the reassignment (%.3f ms); rate of the gather / read rate of icwt = %.2f (all dropped: %.2f, one "
              "bin: %.2f)" % (100 * (med["reassign + bins"] / med["reassign"] - 1), med["reassign + bins"] - med["reassign"],
                              rate["gather"] / rate["icwt"], rate["gather, dropped"] / rate["icwt"], rate["gather, one bin"] / rate["icwt"]), ""]
    for name, _ in calls:
        t = np.array(ctimes[name])
        lines.append("%-55s %8.3f ms (min %.3f max %.3f)" % (name, np.median(t), t.min(), t.max()))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
