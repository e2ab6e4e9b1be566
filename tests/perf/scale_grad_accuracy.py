"""Measures what the bars of tests/scale_grad_common.py are derived from, on the CPU emulation of the library (no GPU needed):

  * fp32: the closed form evaluated in single precision (scale_grad_common.reference32) against the longdouble reference,
    worst |err_j| / S_j over the emulated ABI and hop cases -> MEASURED_REF32 (the fp32 bar is 8 x that, capped at 1e-4);
  * fp64 at set_tolerance(1e-9): the code against the reference over the same cases -> MEASURED_TOL9 (the bar is 4 x that,
    rounded up to a power of ten; a finding if it exceeds 1e3 x the tolerance);
  * for the record: the code itself at the round-off tolerance in both precisions.

    python tests/perf/scale_grad_accuracy.py > profiles/scale_grad_accuracy.txt
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "emu")]

import build_emu  # noqa: E402
import hop_common as hc  # noqa: E402
import scale_grad_common as sc  # noqa: E402
from pycwt_amd import _hip  # noqa: E402


def main():
    lib = _hip.Library(build_emu.build())
    worst = {"ref32": 0.0, "tol9": 0.0, "code64": 0.0, "code32": 0.0}
    print("case                                   ref32/S     code32/S    code64/S    code64@1e-9/S")
    for case in sc.ABI_CASES + sc.HOP_CASES:
        logn, n0, hop, kind, param = case
        N = 1 << logn
        row = {}
        for prec in (32, 64):
            sj, x, G, ref, S = sc.case_reference(case, prec)
            if prec == 32:
                row["ref32"] = sc.ratio(sc.reference32(kind, param, sj, x, G, N, hop), ref, S)
            with hc.Device(lib, N, prec) as dev:
                row["code%d" % prec] = sc.ratio(sc.run(dev, kind, param, sj, x, G, hop)[0], ref, S)
                if prec == 64:
                    dev.plan.set_tolerance(sc.TOL9)
                    row["tol9"] = sc.ratio(sc.run(dev, kind, param, sj, x, G, hop)[0], ref, S)
        for k, v in row.items():
            worst[k] = max(worst[k], v)
        print("%-38s %.3e   %.3e   %.3e   %.3e" % (sc.case_id(case), row["ref32"], row["code32"], row["code64"], row["tol9"]))
    print()
    print("worst reference32 / S            %.3e   -> fp32 bar min(8 x, 1e-4) = %.3e" % (worst["ref32"], min(8 * worst["ref32"], 1e-4)))
    print("worst code fp32 / S              %.3e" % worst["code32"])
    print("worst code fp64 / S (round-off)  %.3e   (bar 1e-12)" % worst["code64"])
    bar9 = sc.pow10_ceil(4 * worst["tol9"])
    print("worst code fp64 / S at 1e-9      %.3e   -> bar 4 x, rounded up to a power of ten = %.0e%s"
          % (worst["tol9"], bar9, "   FINDING: above 1e3 x the tolerance" if bar9 > 1e3 * sc.TOL9 else ""))


if __name__ == "__main__":
    main()
