"""Forward and backward of the differentiable scalogram on one GPU, two routes side by side:

  (a) `pycwt_amd.cwt_torch(x)[0].abs() ** 2` -- W written (16 B per element) and kept by autograd, the cotangent 2 gP W formed by
      torch's elementwise kernels before the adjoint;
  (b) `pycwt_amd.cwt_power_torch(x)[0]`     -- P written by the power row kernels (8 B), nothing but x kept, the backward
      recomputes W under 2 gP in the row kernels' store (cwt_transform_weighted) and runs the same adjoint.

Workloads: config 2 (N = 2^20, 256 scales, fp64 Morlet, accuracy target 1e-9) and a (4, 2^16) complex64 DOG batch (3e-5).  The
routes alternate inside every repeat, after a warm-up that is discarded; every figure is the median of the repeats with their
range.  Per route: forward ms, backward ms, torch's peak allocation over one forward + backward, and the per-kernel-class split of
ONE backward from the plan's own events (option "profile": the library's kernels only -- what torch's elementwise kernels add
to route (a) is its backward time less the sum of the split).

    python tests/perf/power_torch_bench.py [--steps 10] [--warmup 3] [--repeats 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import autograd

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    def stats(v):
        return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def workload(label, shape, real_t, wavelet, tol, grid):
        pycwt_amd.set_tolerance(tol)
        gen = torch.Generator(device="cuda").manual_seed(0)
        x0 = torch.randn(shape, dtype=real_t, device="cuda", generator=gen)
        routes = {
            "a_cwt_torch_abs2": lambda t: pycwt_amd.cwt_torch(t, 1.0, *grid, wavelet)[0].abs().pow(2),
            "b_cwt_power_torch": lambda t: pycwt_amd.cwt_power_torch(t, 1.0, *grid, wavelet)[0],
        }
        out = {"workload": label}
        state, grads = {}, {}
        gP = None
        for name, fn in routes.items():                       # one graph per route, kept for the timed backwards; peak memory
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            x = x0.clone().requires_grad_(True)
            P = fn(x)
            if gP is None:
                gP = torch.randn(P.shape, dtype=real_t, device="cuda", generator=gen)
                base += gP.numel() * gP.element_size()        # (the cotangent is the caller's: not a cost of either route)
            P.backward(gP, retain_graph=True)
            torch.cuda.synchronize()
            out[name] = {"torch_peak_bytes": int(torch.cuda.max_memory_allocated() - base)}
            grads[name] = x.grad.detach().clone()
            x.grad = None
            state[name] = (x, P)
        out["rows"] = int(state["b_cwt_power_torch"][1].shape[-2])
        out["rel_l2_grad_b_vs_a"] = float(torch.linalg.vector_norm((grads["b_cwt_power_torch"] - grads["a_cwt_torch_abs2"]).double())
                                          / torch.linalg.vector_norm(grads["a_cwt_torch_abs2"].double()))

        def forward_of(name):
            def f():
                x = x0.clone().requires_grad_(True)
                routes[name](x)
            return f

        def backward_of(name):
            def f():
                x, P = state[name]
                P.backward(gP, retain_graph=True)
                x.grad = None
            return f

        times = {(n, k): [] for n in routes for k in ("forward", "backward")}
        for rep in range(args.repeats + 1):                   # repeat 0 is the warm-up: discarded
            for name in routes:                               # the routes alternate inside every repeat
                for kind, make in (("forward", forward_of), ("backward", backward_of)):
                    fn = make(name)
                    if rep == 0:
                        for _ in range(args.warmup):
                            fn()
                        torch.cuda.synchronize()
                    else:
                        times[(name, kind)].append(timed(fn))
        for (name, kind), v in times.items():
            out[name][kind] = stats(v)
        eng = next(e for k, e in autograd._engines.items() if k[0] == x0.shape[-1] and k[1] == (64 if real_t == torch.float64 else 32))
        for name in routes:                                   # the library's kernels of ONE backward, by class
            eng.plan.set_option("profile", 1)
            eng.plan.timings()
            backward_of(name)()
            torch.cuda.synchronize()
            split = {k: round(v[0], 4) for k, v in eng.plan.timings().items()}
            eng.plan.set_option("profile", 0)
            out[name]["backward_kernel_classes_ms"] = split
            out[name]["backward_kernel_classes_sum_ms"] = round(sum(split.values()), 4)
        da, db = out["a_cwt_torch_abs2"]["backward"], out["b_cwt_power_torch"]["backward"]
        out["backward_b_minus_a_ms"] = round(db["median_ms"] - da["median_ms"], 4)
        out["backward_spread_ms"] = round(max(da["max_ms"] - da["min_ms"], db["max_ms"] - db["min_ms"]), 4)
        state.clear()
        return out

    m = pycwt_amd.Morlet(6)
    N, rows = 1 << 20, 256
    s0 = 2.0 / m.flambda()
    c2 = (np.log2(N / s0) / (rows - 1), s0, rows - 1)
    results = [workload("config 2: N = 2^20, 256 scales, fp64 Morlet, tolerance 1e-9", (N,), torch.float64, "morlet", 1e-9, c2),
               workload("(4, 2^16) batch, 1/8 octave, complex64 DOG(2), tolerance 3e-5", (4, 1 << 16), torch.float32, "dog", 3e-5,
                        (1 / 8, -1, -1))]
    print(json.dumps({"steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "results": results}, indent=1))


if __name__ == "__main__":
    main()
