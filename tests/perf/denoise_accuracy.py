"""Where the bound of tests/test_shrink_emulated.py and tests/test_shrink_gpu.py on cwt_icwt_shrink comes from: per case of
tests/shrink_common.py (CASES x the three modes x the two precisions) the error max_n |out - ref| / D against the same plan's W
shrunk and summed in long double, D = |coeff| sum_j max_n |W_j| / sqrt(s_j), in units of eps.  The tests assert 4 x the worst
figure per precision (shrink_common.MEASURED, read from the "fp64 / fp32 worst_error_in_eps" lines); a figure above 256 eps is a
defect in the summation.  Runs on the CPU emulation of the HIP runtime (default) or, with --gpu, on the device.  Not collected by
pytest.
Usage: python tests/perf/denoise_accuracy.py [--gpu] [--out profiles/denoise_accuracy.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    sys.path.insert(0, p)


def library(gpu):
    from pycwt_amd import _hip
    if gpu:
        return _hip.load()
    import build_emu
    return _hip.Library(build_emu.build())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import shrink_common as sc
    lib = library(args.gpu)
    lines = ["# cwt_icwt_shrink against the same plan's W shrunk and summed in long double: max_n |out - ref| / D in eps,",
             "# D = |coeff| sum_j max_n |W_j| / sqrt(s_j); W: Morlet(6) of Gaussian noise, n0 = %d on N = %d, %d scales" % (sc.N0, sc.NFFT, sc.ROWS_W),
             "# backend: %s" % lib.backend(), "# precision nrows ncols lambda mode error_in_eps"]
    worst = {}
    for prec in sc.PRECS:
        with sc.Dev(lib, sc.NFFT, prec, max_rows=sc.ROWS_W) as dev:
            for nrows, ncols, pattern in sc.CASES:
                for mode in sc.MODES:
                    err = sc.shrink_error(dev, nrows, ncols, pattern, mode)
                    worst[prec] = max(worst.get(prec, 0.0), err)
                    lines.append("fp%d %4d %5d %-5s %-7s %.4f" % (prec, nrows, ncols, pattern, mode, err))
    for prec in sc.PRECS:
        lines.append("fp%d worst_error_in_eps %.4f" % (prec, worst[prec]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
