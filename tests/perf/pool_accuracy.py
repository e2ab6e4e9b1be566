"""Where the bound of tests/test_pool_emulated.py and tests/test_pool_gpu.py comes from: per case of tests/pool_common.py the worst
per-row ratio max_m |Pbar - ref| / max_m ref of cwt_transform_pool against the same plan's cwt_transform_power output pooled on
the host in long double -- every row form x pool, the polynomial rows by (K', D) at the tolerance 1e-9 and at round-off, the short
signal -- per precision.  The tests assert 4 x the largest figure (pool_common.MEASURED); a figure above 256 eps is a defect in the
summation.  Runs on the CPU emulation of the HIP runtime (default) or, with --gpu, on the device.  Not collected by pytest.
Usage: python tests/perf/pool_accuracy.py [--gpu] [--out profiles/pool_accuracy.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pool_common as pc
    lib = library(args.gpu)
    lines = ["# cwt_transform_pool against the same plan's cwt_transform_power pooled in long double: per-row max_m |Pbar - ref| / max_m ref",
             "# backend: %s" % lib.backend(), "# case pool precision worst_ratio ratio/eps"]
    worst = {64: 0.0, 32: 0.0}

    def record(label, pool, prec, err):
        eps = float(np.finfo(pc.types(prec)[0]).eps)
        worst[prec] = max(worst[prec], float(err))
        lines.append("%-28s %6d %3d %.3e %6.2f" % (label, pool, prec, err, err / eps))

    for prec in (64, 32):
        for form in pc.FORMS:
            for pool, err in pc.check_form(lib, form, prec).items():
                record("form/" + form[0], pool, prec, err)
        for tol, label in ((pc.POLY_TOLERANCE, "poly_rows/1e-9"), (0.0, "poly_rows/round-off")):
            errs, have = pc.check_poly_rows(lib, prec, tol)
            for pool, err in errs.items():
                record(label + "/D<=%d" % max(d for _, d in have), pool, prec, err)
        record("short_signal", pc.SHORT["pool"], prec, pc.check_short_signal(lib, prec))
    for prec in (64, 32):
        eps = float(np.finfo(pc.types(prec)[0]).eps)
        lines.append("# precision %d: worst ratio %.3e = %.2f eps (256 eps = %.3e); the tests assert 4 x: %.3e"
                     % (prec, worst[prec], worst[prec] / eps, 256 * eps, 4 * worst[prec]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
