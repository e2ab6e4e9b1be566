"""The kernels of wavelet shrinkage under the wavefront schedules of the CPU emulation (tests/emu/hipemu.cpp), in the manner of
tests/test_ssq_schedules_emulated.py: forward, reverse and seeded wave orders give the bits of the lockstep order.  The kernels of
cwt_kernels_select.hpp and cwt_kernels_shrink.hpp are called sel_* and shrink_* and are gated here: each of them is launched
under every schedule, and the set of names is read from the headers."""
import os
import re

import numpy as np
import pytest

import shrink_common as sc
from conftest import ROOT
from test_emu_schedules import LOCKSTEP, SCHEDULES, schedule  # noqa: F401  (the fixture that sets and restores the schedule)

KERNELS = {"sel_init", "sel_hist", "sel_pick", "shrink_icwt"}
WAVE_SCHEDULES = [s for s in SCHEDULES if s[1] != LOCKSTEP]


def schedule_case(lib, prec):
    """selections that count, compact and finish in LDS (8 kinds of rows x 4099 columns, reals; 3 rows as complex), one that starts
    compact (257 columns), and the three modes of the shrink-inverse over 9 x 4099 entries: every kernel, as bytes"""
    parts = []
    with sc.Dev(lib, 16, prec, max_rows=16) as dev:
        A, ranks = sc.selection_matrix(8, 4099, prec, 31)
        parts.append(sc.run_select(dev, A, ranks, False))
        parts.append(sc.run_select(dev, A[:3].astype(dev.cplx), ranks[:8], True))
        A, ranks = sc.selection_matrix(8, 257, prec, 32)
        parts.append(sc.run_select(dev, A, ranks, False))
        rng = np.random.default_rng(33)
        Wc = (rng.standard_normal((9, 4099)) + 1j * rng.standard_normal((9, 4099))).astype(dev.cplx)
        lam = sc.thresholds(Wc, prec, "mixed")
        for mode in sc.MODES:
            parts.append(sc.run_shrink(dev, Wc, sc.SJ[:9], lam, mode))
    return np.concatenate([p.view(np.uint8).ravel() for p in parts])


@pytest.mark.parametrize("prec", sc.PRECS)
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, prec):
    schedule(LOCKSTEP)
    base = schedule_case(emu_library, prec)
    for label, kind, seed in WAVE_SCHEDULES:
        schedule(kind, seed)
        emu_library.dll.hipemu_clear_launched()
        got = schedule_case(emu_library, prec)
        log = sc.launch_log(emu_library)
        assert all(any(name in s for s in log) for name in KERNELS), (label, log)
        assert np.array_equal(base, got), label


def test_every_kernel_is_known_to_the_schedule_test():
    """the kernels of the two headers are exactly those the schedule test launches, and none of them is named k_* (those are gated
    by tests/test_emu_schedules.py, whose cases do not launch them)"""
    text = "".join(open(os.path.join(ROOT, "pycwt_amd", "csrc", f)).read() for f in ("cwt_kernels_select.hpp", "cwt_kernels_shrink.hpp"))
    assert set(re.findall(r"__global__[^{;]*?\b((?:sel|shrink)_\w+)\s*\(", text)) == KERNELS
    assert not re.findall(r"__global__[^{;]*?\b(k_\w+)\s*\(", text)
