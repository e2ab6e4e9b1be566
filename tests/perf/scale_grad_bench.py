"""The backward of `pycwt_amd.cwt_torch` with learnable scales on the config-2 workload (N = 2^20, 256 scales, fp64 Morlet, white
noise, the bench's accuracy target 1e-9) on one GPU:

  (a) `scales=` given but not requiring grad: the backward queues the launches of the call without the keyword (compare with
      tests/perf/adjoint_bench.py, "backward_ms_adjoint_poly_1", on the parent commit);
  (b) scales (and f0) requiring grad: one cwt_adjoint_rows_scales call, every row on the general path, with the per-class times
      of one such backward (option "profile"; the sgrad_* kernels are the class "sgrad") -- next to the backward of the call
      without the keyword with adjoint_poly = 0, which is (b) without the spectra of x and the sgrad kernels;
  (c) a full step (forward + backward) with NEW scales every iteration: the grid is classified on the host each time.

    python tests/perf/scale_grad_bench.py [--steps 20] [--warmup 5] [--tolerance 1e-9] > profiles/scale_grad_bench.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tolerance", type=float, default=1e-9)
    args = ap.parse_args()
    import torch
    import pycwt_amd
    from pycwt_amd import autograd

    pycwt_amd.set_tolerance(args.tolerance)
    N, rows = 1 << 20, 256
    m = pycwt_amd.Morlet(6)
    s0 = 2.0 / m.flambda()
    dj = np.log2(N / s0) / (rows - 1)
    x = torch.as_tensor(np.random.default_rng(0).standard_normal(N), device="cuda").requires_grad_(True)
    W0, sj, _, _ = pycwt_amd.cwt_torch(x, 1.0, dj, s0, rows - 1, "morlet")
    gW = torch.randn_like(W0)
    eng = next(e for k, e in autograd._engines.items() if k[0] == N and k[1] == 64)

    def timed(fn, wall=False):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps if wall else a.elapsed_time(b) / args.steps

    def backward_of(W, *leaves):
        def fn():
            W.backward(gW, retain_graph=True)
            for t in (x,) + leaves:
                t.grad = None
        return fn

    def profile(fn):
        eng.plan.set_option("profile", 1)
        fn()
        torch.cuda.synchronize()
        out = {k: round(v[0], 4) for k, v in eng.plan.timings().items()}
        eng.plan.set_option("profile", 0)
        return out

    out = {"workload": f"N = 2^20, {sj.size} scales, fp64 Morlet, tolerance {args.tolerance}",
           "poly_rows": sum(c.startswith("poly") for c in eng.plan.row_classes())}
    out["backward_ms_without_the_keyword"] = timed(backward_of(W0))
    t_fixed = torch.tensor(sj, dtype=torch.float64)
    Wa = pycwt_amd.cwt_torch(x, 1.0, scales=t_fixed)[0]
    out["a_backward_ms_scales_given_no_grad"] = timed(backward_of(Wa))
    out["a_profile"] = profile(backward_of(Wa))
    eng.plan.set_option("adjoint_poly", 0)
    out["backward_ms_without_the_keyword_adjoint_poly_0"] = timed(backward_of(W0))
    eng.plan.set_option("adjoint_poly", 1)
    t = t_fixed.clone().requires_grad_(True)
    f0 = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
    Wb = pycwt_amd.cwt_torch(x, 1.0, scales=t, f0=f0)[0]
    out["b_backward_ms_scales_and_f0_grad"] = timed(backward_of(Wb, t, f0))
    out["b_profile"] = profile(backward_of(Wb, t, f0))
    Wb.backward(gW, retain_graph=True)
    out["b_grad_scales_finite"] = bool(torch.isfinite(t.grad).all())
    step = [0]

    def full_step():
        step[0] += 1
        ts = (t_fixed * (1.0 + 1e-6 * step[0])).requires_grad_(True)       # a new grid: classified on the host
        W = pycwt_amd.cwt_torch(x, 1.0, scales=ts)[0]
        W.backward(gW)
        x.grad = None

    def fixed_step():
        W = pycwt_amd.cwt_torch(x, 1.0, scales=t)[0]
        W.backward(gW)
        x.grad = t.grad = None
    out["c_step_ms_wall_fixed_scales"] = timed(fixed_step, wall=True)
    out["c_step_ms_wall_new_scales_every_step"] = timed(full_step, wall=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
