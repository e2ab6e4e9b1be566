"""Measurements behind tests/test_switch_scales_*.py (tests/switch_common.py): the switch pairs of the row classifier per case, the
families they belong to, and the worst per-row error against the oracle per (N, precision, mother, target, family).

    python tests/perf/switch_scales.py --backend emu --json emu.json            # the cases of the emulated file (minutes)
    python tests/perf/switch_scales.py --backend hip --json hip.json            # ... of the GPU file, N = 2^20 included
    python tests/perf/switch_scales.py --table emu.json hip.json > profiles/switch_scales.txt
    python tests/perf/switch_scales.py --backend emu --families                 # the FAMILIES literal of switch_common.py

--families launches nothing (find_switches and one Plan.classify over the pair scales per case), so it also covers N = 2^20 on
the emulator; paste its output over the FAMILIES block of tests/switch_common.py after a retuning that moves the switches.
"""
import argparse
import json
import os
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import switch_common as sc  # noqa: E402
from oracle import cwt_oracle as orc  # noqa: E402
from pycwt_amd import _hip  # noqa: E402


def library(backend):
    if backend == "emu":
        import build_emu
        return _hip.Library(build_emu.build())
    lib = _hip.load()
    assert lib.backend() == "hip-gfx950" and lib.device_count() >= 1
    return lib


def all_cases(sizes):
    """(case, with_signal): the value cases, the spectrum-only cases, and with 20 among the sizes the flagship cases"""
    out = [(c, True) for logn in (15, 18) if logn in sizes for c in sc.value_cases(logn)]
    out += [(c, False) for c in sc.rows_cases() if c[0] in sizes]
    if 20 in sizes:
        out += [(c, True) for c in sc.flagship_cases()]
    return out


def most_of(logn):
    return sc.FLAGSHIP_ROWS // 2 if logn == 20 else None


def families(lib, sizes):
    print("FAMILIES = {")
    for (logn, prec, kind, param, target, signal), with_signal in all_cases(sizes):
        if signal != "white":
            continue
        N = 1 << logn
        n0 = N - sc.N0_OFF
        plan = _hip.Plan(N, prec, max_rows=sc.MAX_ROWS, lib=lib, options=dict(sc.SIZES[logn] or {}))
        try:
            plan.set_tolerance(target)
            pairs = sc.find_switches(plan, kind, param, n0, n0, with_signal)
            if most_of(logn):
                pairs = sc.thin(pairs, most_of(logn))
            joint = plan.classify(kind, param, 1.0, sc.pair_scales(pairs), n0, with_signal)
        finally:
            plan.close()
        fams = sorted({sc.family(joint[2 * i], joint[2 * i + 1]) for i in range(len(pairs)) if joint[2 * i] != joint[2 * i + 1]})
        key = (logn, prec, sc.mother_id(kind, param), target, with_signal)
        print("    %r: {" % (key,))
        print(textwrap.fill(", ".join(repr(f) for f in fams), 128, initial_indent="        ", subsequent_indent="        ") + "},")
    print("}")


def measure(lib, sizes, path):
    records = []
    for (logn, prec, kind, param, target, signal), with_signal in all_cases(sizes):
        N = 1 << logn
        r = sc.run_pairs(lib, N, N - sc.N0_OFF, prec, kind, param, sc.SIZES[logn], target, signal, with_signal=with_signal,
                         most=most_of(logn))
        keep = r.straddling()
        rec = {"logn": logn, "prec": prec, "mother": sc.mother_id(kind, param), "target": target, "signal": signal,
               "with_signal": with_signal, "pairs": len(r.pairs), "kept": len(keep), "worst": list(r.worst()),
               "families": {"%s <-> %s" % f: e for f, e in sc.family_errors(r, keep).items()}}
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(path, "w") as f:                       # (after every case: a long run leaves what it has)
            json.dump({"backend": lib.backend(), "records": records}, f, indent=0)


def table(paths):
    runs = [json.load(open(p)) for p in paths]
    names = [r["backend"] for r in runs]
    cells = {}
    for k, run in enumerate(runs):
        for rec in run["records"]:
            head = (rec["logn"], rec["prec"], rec["mother"], rec["target"], rec["signal"], rec["with_signal"])
            for fam, e in list(rec["families"].items()) + [("(worst row: %s)" % rec["worst"][1], rec["worst"][2])]:
                fam = "(worst row of the case)" if fam.startswith("(worst") else fam
                cells.setdefault(head, {}).setdefault(fam, [None] * len(runs))[k] = e
            cells[head].setdefault("(pairs found / still straddling)", [None] * len(runs))[k] = (rec["pairs"], rec["kept"])
    print("Worst per-row error max|dW| / max|oracle row| at the classifier's switch pairs, per case and family of switches")
    print("(tests/perf/switch_scales.py; the cases and bounds of tests/test_switch_scales_emulated.py / _gpu.py).")
    print("entry: cwt_transform, or rows = forward_fft + cwt_transform_rows.  target 0 = round-off.")
    print()
    print("%-5s %-4s %-8s %-7s %-9s %-5s %-44s %s" % ("N", "prec", "mother", "target", "signal", "entry", "family",
                                                       "  ".join("%-14s" % n for n in names)))
    for head in sorted(cells, key=lambda h: (h[0], -h[1], h[2], h[3], h[4], not h[5])):
        for fam in sorted(cells[head], key=lambda f: (f.startswith("("), f)):
            vals = cells[head][fam]
            txt = "  ".join("%-14s" % ("-" if v is None else ("%d / %d" % tuple(v) if isinstance(v, (list, tuple)) else "%.3e" % v))
                            for v in vals)
            print("2^%-3d fp%-2d %-8s %-7g %-9s %-5s %-44s %s" % (head[0], head[1], head[2], head[3], head[4],
                                                                "call" if head[5] else "rows", fam, txt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["emu", "hip"], default="emu")
    ap.add_argument("--sizes", default=None, help="comma-separated log2 N (default: 15,18 and, on hip or with --families, 20)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--families", action="store_true")
    ap.add_argument("--table", nargs="+")
    a = ap.parse_args()
    if a.table:
        return table(a.table)
    sizes = [int(s) for s in a.sizes.split(",")] if a.sizes else ([15, 18, 20] if a.backend == "hip" or a.families else [15, 18])
    lib = library(a.backend)
    if a.families:
        return families(lib, sizes)
    assert a.json, "--json FILE"
    measure(lib, sizes, a.json)


if __name__ == "__main__":
    main()
