"""The backward of wavelet shrinkage on one GPU, alternated in one process, at config 2 (N = 2^20, 256 scales, fp64 Morlet(6),
tau = 1e-9), white noise, universal soft thresholds:

  icwt                 cwt_icwt_reduce over W (k_icwt): the read-rate yardstick of this run
  shrink soft          cwt_icwt_shrink (the forward of the layer)
  adjoint <mode>       cwt_icwt_shrink_adjoint with glambda, G beside W (one read and one write of W, gy re-read by every row)
  half kept: <mode>    the same with the medians of |W_j| as thresholds: half of every row takes the arithmetic of a kept entry
  adjoint soft, no gl  the same without glambda (no LDS tree, no shgrad_sum)
  adjoint in place     G_dev = W_dev
  adjoint plain        lambda_dev = NULL: W is not read -- one write of W and the re-reads of gy alone
  torch backward       the vector-Jacobian product of "half kept: soft" by torch autograd through W * clamp(1 - lam / |W|, 0) and the
                       weighted sum
  step denoise_torch   forward + backward of denoise_torch with learnable thresholds (host clock, synchronised)
  step cwt_torch+ops   the same step as cwt_torch + the torch operations above

Device events on torch's current stream around each kernel step; 3 warm-up rounds, then `--reps` rounds of all steps in turn;
medians and the spread.  The adjoint is set against the traffic of one read and one write of W at the rate `icwt` reaches in this
run, with and without rows x N x 8 bytes for gy read from memory by every row: which of the two the time sits at shows whether gy
stays in cache.  Peak memory from torch's counter (the plan's own scratch is not in it).  There is no pass mark: the numbers are a
record.  Not collected by pytest.
Usage: python tests/perf/shrink_grad_bench.py [--reps 20] [--out profiles/shrink_grad_bench.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shrink_grad_bench.txt"))
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("shrink_grad_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    reps = args.reps
    mother = pycwt_amd.Morlet(6)
    sj = scale_grid(mother.flambda())
    dj = float(np.log2(N / sj[0]) / (ROWS - 1))
    dev = torch.device("cuda:0")
    xs = np.random.default_rng(1234).standard_normal(N)
    x = torch.from_numpy(xs).to(dev)
    plan = _hip.Plan(N, 64, max_rows=ROWS, lib=lib, options={"tolerance": TAU})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    xh = torch.empty(N, dtype=torch.complex128, device=dev)
    W = torch.empty((ROWS, N), dtype=torch.complex128, device=dev)
    G = torch.empty((ROWS, N), dtype=torch.complex128, device=dev)
    stats = torch.empty((ROWS, 2), dtype=torch.float64, device=dev)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    gl = torch.empty(ROWS, dtype=torch.float64, device=dev)
    gy = torch.from_numpy(np.random.default_rng(5).standard_normal(N)).to(dev)
    ranks = [N // 2 - 1, N // 2]
    c = float(np.sqrt(np.log(4.0)))
    w_t = torch.from_numpy(1 / np.sqrt(sj)).to(dev)
    plan.transform(x.data_ptr(), N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N)
    plan.row_order_statistics(W.data_ptr(), True, N, N, ROWS, ranks, stats.data_ptr(), 2)
    lam = (0.5 * (stats[:, 0].sqrt() + stats[:, 1].sqrt()) / c * float(np.sqrt(2 * np.log(N)))).contiguous()
    torch.cuda.synchronize()
    lam_half = (0.5 * (stats[:, 0].sqrt() + stats[:, 1].sqrt())).contiguous()      # the medians themselves: half of every row kept
    kept = float((W.abs() > lam[:, None]).double().mean())
    kept_half = float((W.abs() > lam_half[:, None]).double().mean())
    W2 = W.clone()                                                    # the buffer of the in-place call (overwritten by every call)
    held = {}

    def adjoint(mode, lam_ptr, gl_ptr, src=W, dst=G):
        plan.icwt_shrink_adjoint(src.data_ptr(), N, N, sj, lam_ptr, mode, 1.0, gy.data_ptr(), dst.data_ptr(), N, gl_ptr)

    def torch_backward():
        Wl = W.detach().requires_grad_(True)
        ll = lam_half.detach().requires_grad_(True)
        y = (Wl.real * torch.clamp(1 - ll[:, None] / Wl.abs(), min=0) * w_t[:, None]).sum(dim=0)
        held["gW"], held["gl"] = torch.autograd.grad(y, (Wl, ll), gy)

    steps = [("icwt", lambda: plan.icwt_reduce(W.data_ptr(), N, N, sj, 1.0, out.data_ptr())),
             ("shrink soft", lambda: plan.icwt_shrink(W.data_ptr(), N, N, sj, lam.data_ptr(), "soft", 1.0, out.data_ptr()))]
    steps += [("adjoint " + m, lambda m=m: adjoint(m, lam.data_ptr(), gl.data_ptr())) for m in ("hard", "soft", "garrote")]
    steps += [("half kept: " + m, lambda m=m: adjoint(m, lam_half.data_ptr(), gl.data_ptr())) for m in ("soft", "garrote")]
    steps += [("adjoint soft, no gl", lambda: adjoint("soft", lam.data_ptr(), None)),
              ("adjoint in place", lambda: adjoint("soft", lam.data_ptr(), gl.data_ptr(), W2, W2)),
              ("adjoint plain", lambda: adjoint(0, None, None)),
              ("torch backward", torch_backward)]
    for _ in range(3):
        for _, fn in steps:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in steps}
    for _ in range(reps):
        for name, fn in steps:
            times[name].append(event_ms(torch, fn))
    # the two routes agree
    adjoint("soft", lam_half.data_ptr(), gl.data_ptr())
    torch.cuda.synchronize()
    g_err = float((G - held["gW"]).abs().max() / held["gW"].abs().max())
    l_err = float(((gl - held["gl"]).abs() / held["gl"].abs().clamp(min=1e-300)).max())
    held.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch_backward()
    torch.cuda.synchronize()
    peak_torch = torch.cuda.max_memory_allocated() - base
    held.clear()
    matrix = ROWS * N * 16
    med = {name: float(np.median(times[name])) for name, _ in steps}
    rate = matrix / (med["icwt"] * 1e-3)
    lines = ["Backward of wavelet shrinkage: N = 2^20, 256 scales, fp64 Morlet(6), tau = 1e-9, white noise, universal soft thresholds "
             "(%.4f %% of the entries kept; \"half kept\": the medians as thresholds, %.1f %%), %s, build %s." % (100 * kept, 100 * kept_half, torch.cuda.get_device_name(0), lib.build_id()),
             "Alternated in one process, %d rounds after 3 warm-up rounds; medians (min, max) of device events.  "
             "Written by tests/perf/shrink_grad_bench.py." % reps, ""]
    for name, _ in steps:
        t = np.array(times[name])
        lines.append("%-20s %8.3f ms (min %.3f max %.3f)" % (name, np.median(t), t.min(), t.max()))
    t_rw, t_gy = 2 * matrix / rate * 1e3, (2 * matrix + ROWS * N * 8) / rate * 1e3
    lines += ["", "icwt reads W (%.2f GB) at %.2f TB/s.  One read and one write of W at that rate: %.3f ms; with gy (8 MB) read from memory by "
              "every row (+ %.2f GB): %.3f ms." % (matrix / 1e9, rate / 1e12, t_rw, ROWS * N * 8 / 1e9, t_gy),
              "adjoint soft with glambda %.3f ms = %.2f of the first, %.2f of the second; without glambda %.3f ms; in place %.3f ms."
              % (med["adjoint soft"], med["adjoint soft"] / t_rw, med["adjoint soft"] / t_gy, med["adjoint soft, no gl"], med["adjoint in place"]),
              "adjoint plain (one write of W, gy re-read by every row, no read of W): %.3f ms = %.2f of one pass over W at icwt's rate."
              % (med["adjoint plain"], med["adjoint plain"] / (matrix / rate * 1e3)),
              "torch backward / half kept soft: %.1f x; peak memory of the torch route above W, lam and gy: %.2f GB (W is %.2f GB); the "
              "kernel route holds G (%.2f GB; none in place).  The two routes agree: G to %.1e of its peak, glambda to %.1e relative."
              % (med["torch backward"] / med["half kept: soft"], peak_torch / 1e9, matrix / 1e9, matrix / 1e9, g_err, l_err)]
    plan.set_option("profile", 1)                                   # per kernel class, every kernel alone on the stream
    for name, fn in steps[3:7]:
        for _ in range(3):
            fn()
        plan.timings()
        for _ in range(reps):
            fn()
        per = {k: (v[0] / reps * 1e3, v[1] // reps) for k, v in plan.timings().items()}
        lines.append("per kernel class, %-20s (profile: serialised): " % name +
                     "  ".join("%s %.1f us in %d timed group(s)" % (k, per[k][0], per[k][1]) for k in sorted(per)))
    plan.close()
    del W, W2, G, xh
    torch.cuda.empty_cache()
    # the whole step: forward + backward, learnable thresholds, host clock around a synchronised step
    pycwt_amd.set_tolerance(TAU)
    kw = dict(dj=dj, s0=sj[0], J=ROWS - 1, wavelet=mother)
    lam_p = lam.detach().clone().requires_grad_(True)
    xg = x.detach().clone().requires_grad_(True)
    coeff = float(np.real(dj / (mother.cdelta * mother.psi(0))))

    def step_kernels():
        y = pycwt_amd.denoise_torch(xg, 1.0, threshold=lam_p, mode="soft", **kw)[0]
        (y * gy).sum().backward()

    def step_torch():
        Wt = pycwt_amd.cwt_torch(xg, 1.0, **kw)[0]
        y = (Wt.real * torch.clamp(1 - lam_p[:, None] / Wt.abs(), min=0) * w_t[:, None]).sum(dim=0) * coeff
        (y * gy).sum().backward()

    whole = {}
    for name, fn in (("step denoise_torch", step_kernels), ("step cwt_torch+ops", step_torch)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        grads = (xg.grad.clone(), lam_p.grad.clone())
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(max(5, reps // 2)):
            xg.grad = lam_p.grad = None
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        whole[name] = (np.array(ts), torch.cuda.max_memory_allocated() - base, (xg.grad.clone(), lam_p.grad.clone()))
        del grads
    for name, (ts, peak, _) in whole.items():
        lines.append("%-20s %8.3f ms (min %.3f max %.3f) forward + backward, host clock; peak memory above the resident tensors %.2f GB"
                     % (name, np.median(ts), ts.min(), ts.max(), peak / 1e9))
    ga, gb = whole["step denoise_torch"][2], whole["step cwt_torch+ops"][2]
    lines.append("the two steps agree: x.grad to %.1e of its peak, lam.grad to %.1e of its peak"
                 % (float((ga[0] - gb[0]).abs().max() / gb[0].abs().max()), float((ga[1] - gb[1]).abs().max() / gb[1].abs().max())))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
