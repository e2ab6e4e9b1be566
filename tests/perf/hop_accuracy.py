"""Where the bounds of tests/test_hop_emulated.py and tests/test_hop_gpu.py come from: per case of tests/hop_common.py the
per-row error of the EXISTING cwt_transform at round-off and of cwt_transform_hop, both against the oracle (float64) on the
same inputs, relative to the row's own peak in the undecimated oracle row; and the gradient of a loss on W[:, ::h] through the
existing cwt_torch and through cwt_torch(hop=h) against the float64 NumPy adjoint.  The bounds are 4 x the largest figure of
the existing route per precision.  Runs on the CPU emulation of the HIP runtime (default) or, with --gpu, on the device.  Not
collected by pytest.  Usage: python tests/perf/hop_accuracy.py [--gpu] [--out profiles/hop_accuracy.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)


def library(gpu):
    from pycwt_amd import _hip
    if gpu:
        return _hip.load()
    import build_emu
    return _hip.Library(build_emu.build())


def grad_case(lib, gpu, prec, N=1 << 15, n0=(1 << 15) - 77, hop=16):
    """(error of the existing route, error of the hop route, error between them): gradient of sum Re(conj(C) W[:, ::h]) w.r.t. x"""
    import torch
    import pycwt_amd
    from pycwt_amd import _hip, autograd
    from oracle import cwt_oracle as orc
    _hip._default = lib
    autograd._engines.clear()
    real_t = torch.float64 if prec == 64 else torch.float32
    device = "cuda" if gpu else "cpu"
    rng = np.random.default_rng(41)
    x0 = torch.as_tensor(rng.standard_normal(n0), dtype=real_t, device=device)
    m = pycwt_amd.Morlet(6)
    xa = x0.clone().requires_grad_(True)
    W, sj, _, _ = pycwt_amd.cwt_torch(xa, 1.0, 1 / 4, wavelet=m)
    nch = -(-n0 // hop)
    Cn = rng.standard_normal((len(sj), nch)) + 1j * rng.standard_normal((len(sj), nch))
    Ct = torch.as_tensor(Cn, device=device).to(W.dtype)
    (W[:, ::hop].conj() * Ct).real.sum().backward()
    xb = x0.clone().requires_grad_(True)
    Wh = pycwt_amd.cwt_torch(xb, 1.0, 1 / 4, wavelet=m, hop=hop)[0]
    (Wh.conj() * Ct).real.sum().backward()
    # float64 reference: Re A^H of the cotangent, zero between the kept columns
    G = np.zeros((len(sj), n0), dtype=np.complex128)
    G[:, ::hop] = Ct.cpu().numpy().astype(np.complex128)
    bank = orc.filter_bank(np.asarray(sj, dtype=float), orc.angular_freqs(N, 1.0), N, orc.Mother(orc.MORLET, 6), True)
    ref = np.real(np.fft.ifft((np.conj(bank) * np.fft.fft(G, n=N, axis=1)).sum(axis=0)))[:n0]
    ga, gb = xa.grad.cpu().numpy().astype(np.float64), xb.grad.cpu().numpy().astype(np.float64)

    def rel(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    for e in autograd._engines.values():
        e.plan.close()
    autograd._engines.clear()
    return rel(ga, ref), rel(gb, ref), rel(gb, ga)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hop_accuracy.txt"))
    args = ap.parse_args()
    import hop_common as hc
    lib = library(args.gpu)
    lines = ["Per-row errors against the oracle (float64), max over the rows of max|W - W_oracle| / max|W_oracle row|, on %s." % lib.backend(),
             "existing = cwt_transform at round-off (all columns), hop = cwt_transform_hop against columns ::hop of the same oracle rows.",
             "Cases, scale grid and signals: tests/hop_common.py.  Written by tests/perf/hop_accuracy.py.", "",
             "%-34s %4s %12s %12s %7s" % ("case", "prec", "existing", "hop", "ratio")]
    worst = {64: [0.0, 0.0], 32: [0.0, 0.0]}
    for prec in (64, 32):
        for c in hc.CASES:
            logn, hop, n0, kind, param = c
            sj, ref, peak = hc.reference(logn, n0, kind, param, prec)
            x = hc.signal(n0, prec)
            with hc.Device(lib, 1 << logn, prec) as dev:
                e_full = hc.row_error(hc.run_full(dev, x, kind, param, sj), ref, peak)
                e_hop = hc.row_error(hc.run_hop(dev, x, kind, param, sj, hop), ref[:, ::hop], peak)
            worst[prec] = [max(worst[prec][0], e_full), max(worst[prec][1], e_hop)]
            lines.append("%-34s %4d %12.3e %12.3e %7.2f" % (hc.case_id(c), prec, e_full, e_hop, e_hop / e_full))
    lines += ["", "largest per precision, and the bound of the hop rows = 4 x existing:"]
    for prec in (64, 32):
        lines.append("  fp%d  existing %.3e   hop %.3e   bound %.3e" % (prec, worst[prec][0], worst[prec][1], 4 * worst[prec][0]))
    lines += ["", "Gradient of sum Re(conj(C) W[:, ::16]) at nfft = 2^15, n0 = 2^15 - 77, Morlet(6), dj = 1/4: relative L2 error against the",
              "float64 NumPy adjoint, through the existing cwt_torch + slice, through cwt_torch(hop=16), and between the two routes:"]
    for prec in (64, 32):
        ea, eb, ab = grad_case(lib, args.gpu, prec)
        lines.append("  fp%d  existing %.3e   hop %.3e   hop vs existing %.3e   bound (4 x existing) %.3e" % (prec, ea, eb, ab, 4 * ea))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
