"""Forward and backward of `pycwt_amd.cwt_torch` on the config-2 workload (N = 2^20, 256 scales, fp64 Morlet, white noise, the
bench's accuracy target 1e-9) on one GPU, the backward with the transpose of the polynomial form (option adjoint_poly = 1, the
default) and with every row through the general path (0); per-kernel-class times of one backward of each (option "profile").

    python tests/perf/adjoint_bench.py [--steps 20] [--warmup 5] [--tolerance 1e-9]
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
    W, sj, _, _ = pycwt_amd.cwt_torch(x, 1.0, dj, s0, rows - 1, "morlet")
    gW = torch.randn_like(W)
    eng = next(e for k, e in autograd._engines.items() if k[0] == N and k[1] == 64)
    classes = eng.plan.row_classes()
    n_poly = sum(c.startswith("poly") for c in classes)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.steps

    def forward():
        with torch.no_grad():
            pycwt_amd.cwt_torch(x.detach(), 1.0, dj, s0, rows - 1, "morlet")

    def backward():
        W.backward(gW, retain_graph=True)
        x.grad = None

    out = {"workload": f"N = 2^20, {sj.size} scales, fp64 Morlet, tolerance {args.tolerance}", "poly_rows": n_poly,
           "forward_ms": timed(forward)}
    grads = {}
    for flag in (1, 0):
        eng.plan.set_option("adjoint_poly", flag)
        out[f"backward_ms_adjoint_poly_{flag}"] = timed(backward)
        W.backward(gW, retain_graph=True)
        grads[flag] = x.grad.detach().cpu().numpy()
        x.grad = None
        eng.plan.set_option("profile", 1)
        backward()
        torch.cuda.synchronize()
        out[f"profile_adjoint_poly_{flag}"] = {k: round(v[0], 4) for k, v in eng.plan.timings().items()} \
            if hasattr(eng.plan, "timings") else None
        eng.plan.set_option("profile", 0)
    eng.plan.set_option("adjoint_poly", 1)
    out["rel_l2_poly_vs_general"] = float(np.linalg.norm(grads[1] - grads[0]) / np.linalg.norm(grads[0]))
    out["backward_over_forward"] = out["backward_ms_adjoint_poly_1"] / out["forward_ms"]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
