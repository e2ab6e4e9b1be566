"""W step against power step (cwt_transform vs cwt_transform_power) on one GPU, alternated in one process.

Configs (BASELINE): c2 = fp64 Morlet(6), N = 2^20, 256 scales, tau = 1e-9; c3_paul / c3_dog = fp32, tau = 3e-5; c4 = the batch of
1024 signals x 2^16 x 128 Morlet scales (cwt_transform_batch vs cwt_transform_batch_power; --c4-signals to shrink it).  Each
run: warm-up of both steps, then `--reps` rounds of (W step, power step) timed with device events, `--runs` runs.  Reports ms
and achieved bytes/s against the algorithmic bytes of each output (16 / 8 B per element of W / P in fp64, 8 / 4 in fp32, plus
the signal).  Not collected by pytest.  Usage: python tests/perf/power_bench.py [--configs c2,c3_paul,c3_dog,c4] [--out F]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": (0, 6.0, 64, 1e-9), "c3_paul": (1, 4.0, 32, 3e-5), "c3_dog": (2, 2.0, 32, 3e-5)}


def scale_grid(N, flambda, rows):
    s0 = 2 / flambda
    return s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))


def flambda(kind, p):
    from pycwt_amd import mothers
    return (mothers.Morlet(p), mothers.Paul(int(p)), mothers.DOG(int(p)))[kind].flambda()


def timed(torch, fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    out = []
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    for a, b in ev:
        out.append(a.elapsed_time(b))
    return out


def bench_pair(torch, step_w, step_p, bytes_w, bytes_p, runs, reps):
    for _ in range(3):
        step_w()
        step_p()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(runs):
        for _ in range(reps):                 # alternated: W, power, W, power ...
            tw = timed(torch, step_w, 1)[0]
            tp = timed(torch, step_p, 1)[0]
            rounds.append((tw, tp))
    tw = np.array([r[0] for r in rounds])
    tp = np.array([r[1] for r in rounds])
    return {"w_ms": tw.tolist(), "power_ms": tp.tolist(), "w_ms_median": float(np.median(tw)),
            "power_ms_median": float(np.median(tp)), "ratio_median": float(np.median(tp / tw)),
            "power_faster_every_round": bool((tp < tw).all()),
            "w_bytes": bytes_w, "power_bytes": bytes_p,
            "w_TBps": bytes_w / (np.median(tw) * 1e-3) / 1e12, "power_TBps": bytes_p / (np.median(tp) * 1e-3) / 1e12}


def single(torch, lib, name, runs, reps):
    from pycwt_amd import _hip
    kind, param, prec, tau = CONFIGS[name]
    N, rows = 1 << 20, 256
    sj = scale_grid(N, flambda(kind, param), rows)
    from oracle import cwt_oracle as orc
    sj = sj[~orc.dropped_rows(sj, 1.0, orc.Mother(kind, param))]
    real_t, cplx_t = (torch.float64, torch.complex128) if prec == 64 else (torch.float32, torch.complex64)
    es = 8 if prec == 64 else 4
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.random.default_rng(1234).standard_normal(N)).to(dev, real_t)
    xh = torch.empty(N, dtype=cplx_t, device=dev)
    W = torch.empty((len(sj), N), dtype=cplx_t, device=dev)
    P = torch.empty((len(sj), N), dtype=real_t, device=dev)
    plan = _hip.Plan(N, prec, max_rows=rows, lib=lib, options={"tolerance": tau})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)

    def sw():
        plan.transform(x.data_ptr(), N, kind, param, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N)

    def sp():
        plan.transform_power(x.data_ptr(), N, kind, param, 1.0, sj, xh.data_ptr(), P.data_ptr(), N, N)
    r = bench_pair(torch, sw, sp, len(sj) * N * 2 * es + N * es, len(sj) * N * es + N * es, runs, reps)
    Wh, Ph = W.cpu().numpy(), P.cpu().numpy()
    ref = Wh.real.astype(np.float64) ** 2 + Wh.imag.astype(np.float64) ** 2
    r["max_row_err_vs_abs2_W"] = float((np.abs(Ph - ref).max(axis=1) / ref.max(axis=1)).max())
    r["rows"], r["split"] = len(sj), plan.last_split()
    plan.close()
    return r


def batch(torch, lib, nb, runs, reps):
    from pycwt_amd import _hip
    N, rows = 1 << 16, 128
    sj = scale_grid(N, flambda(0, 6.0), rows)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    X = torch.randn(nb, N, dtype=torch.float64, device=dev, generator=g)
    xh = torch.empty(nb, N, dtype=torch.complex128, device=dev)
    W = torch.empty(nb, rows, N, dtype=torch.complex128, device=dev)
    P = torch.empty(nb, rows, N, dtype=torch.float64, device=dev)
    plan = _hip.Plan(N, 64, max_rows=nb * rows, lib=lib, options={"tolerance": 1e-9})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)

    def sw():
        plan.transform_batch(X.data_ptr(), nb, N, N, 0, 6.0, 1.0, sj, xh.data_ptr(), W.data_ptr(), N, N)

    def sp():
        plan.transform_batch_power(X.data_ptr(), nb, N, N, 0, 6.0, 1.0, sj, xh.data_ptr(), P.data_ptr(), N, N)
    r = bench_pair(torch, sw, sp, nb * rows * N * 16 + nb * N * 8, nb * rows * N * 8 + nb * N * 8, runs, reps)
    w0, p0 = W[0, :8].cpu().numpy(), P[0, :8].cpu().numpy()
    ref = w0.real ** 2 + w0.imag ** 2
    r["max_row_err_vs_abs2_W_sampled"] = float((np.abs(p0 - ref).max(axis=1) / ref.max(axis=1)).max())
    r["signals"] = nb
    plan.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c3_paul,c3_dog,c4")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--c4-signals", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from pycwt_amd import _hip
    if not torch.cuda.is_available():
        sys.exit("power_bench: no GPU visible (a timing needs the device)")
    lib = _hip.load()
    res = {}
    for name in args.configs.split(","):
        res[name] = batch(torch, lib, args.c4_signals, args.runs, args.reps) if name == "c4" else single(torch, lib, name, args.runs,
                                                                                                         args.reps)
        r = res[name]
        print(f"{name}: W {r['w_ms_median']:.3f} ms ({r['w_TBps']:.2f} TB/s), power {r['power_ms_median']:.3f} ms "
              f"({r['power_TBps']:.2f} TB/s), power/W {r['ratio_median']:.3f}, faster every round: {r['power_faster_every_round']}",
              flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
