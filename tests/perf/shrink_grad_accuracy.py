"""The measured worst cases of cwt_icwt_shrink_adjoint beside the bounds that tests/test_shrink_grad_emulated.py and
tests/test_shrink_grad_gpu.py assert: per case of tests/shrink_grad_common.py (CASES x the three modes x the two precisions) the
largest error of G relative to |t| and of glambda relative to sum |term| against the closed form in long double, in units of
u = eps / 2.  The bounds are COUNTED (the module docstring of shrink_grad_common.py), not read from this record; a case beyond its
bound stops the script.  Runs on the CPU emulation of the HIP runtime (default) or, with --gpu, on the device.  Not collected by
pytest.
Usage: python tests/perf/shrink_grad_accuracy.py [--gpu] [--out profiles/shrink_grad_accuracy.txt]
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
    import shrink_grad_common as gc
    lib = library(args.gpu)
    lines = ["# cwt_icwt_shrink_adjoint against the closed form in long double on the inputs rounded to T, every entry:",
             "# G: max |G - ref| / |t| (the larger of the two components), glambda: max_j |glambda_j - sum term| / sum |term|, in u = eps / 2",
             "# backend: %s" % lib.backend(), "# precision nrows ncols lambda mode G_in_u G_bound glambda_in_u glambda_bound"]
    worst = {}
    cases = list(gc.CASES) + ([gc.LARGE + ("mixed",)] if args.gpu else [])
    for prec in gc.PRECS:
        with gc.Dev(lib, 16, prec, max_rows=16) as dev:
            for nrows, ncols, pattern in cases:
                for mode in gc.MODES:
                    g, l = gc.check_closed_form(dev, nrows, ncols, pattern, mode)
                    key = (prec, mode)
                    worst[key] = (max(worst.get(key, (0, 0))[0], g), max(worst.get(key, (0, 0))[1], l))
                    lines.append("fp%d %4d %6d %-5s %-7s %7.3f %3d %7.3f %6.2f" % (prec, nrows, ncols, pattern, mode, g, gc.G_BOUND[mode], l,
                                                                                 gc.glambda_bound_units(mode, ncols, dev.eps)))
    for (prec, mode), (g, l) in sorted(worst.items()):
        lines.append("fp%d %-7s worst_in_u G %.3f (bound %d) glambda %.3f (bound at 4099 columns %.2f)"
                     % (prec, mode, g, gc.G_BOUND[mode], l, gc.glambda_bound_units(mode, 4099, gc.types(prec)[2])))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
