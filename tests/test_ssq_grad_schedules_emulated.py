"""The kernels of the synchrosqueezed transform's gradient under the wavefront schedules of the CPU emulation (tests/emu/hipemu.cpp),
in the manner of tests/test_ssq_schedules_emulated.py: forward, reverse and seeded wave orders give the bits of the lockstep order.
The kernels of cwt_kernels_ssq_grad.hpp are called ssqg_* and are gated here: each of them is launched under every schedule, and
the set of names is read from the header."""
import os
import re

import numpy as np
import pytest

import ssq_common as sc
import ssq_grad_common as gc
from conftest import ROOT
from test_emu_schedules import LOCKSTEP, SCHEDULES, schedule  # noqa: F401  (the fixture that sets and restores the schedule)

WAVE_SCHEDULES = [s for s in SCHEDULES if s[1] != LOCKSTEP]


@pytest.mark.parametrize("prec", sc.PRECS)
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, prec):
    schedule(LOCKSTEP)
    base = gc.schedule_case(emu_library, prec)
    assert {"waves", "waves-reverse"} <= {s[0] for s in WAVE_SCHEDULES} and any(s[0].startswith("waves-seeded") for s in WAVE_SCHEDULES)
    for label, kind, seed in WAVE_SCHEDULES:
        schedule(kind, seed)
        emu_library.dll.hipemu_clear_launched()
        got = gc.schedule_case(emu_library, prec)
        log = sc.launch_log(emu_library)
        assert all(any(name in s for s in log) for name in gc.GRAD_KERNELS), (label, log)
        assert np.array_equal(base, got), label


def test_every_ssq_grad_kernel_is_known_to_the_schedule_test():
    """the kernels of cwt_kernels_ssq_grad.hpp are exactly those the schedule test launches, and none of them is named k_* (those
    are gated by tests/test_emu_schedules.py, whose cases do not launch them)"""
    text = open(os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_ssq_grad.hpp")).read()
    assert text.count("__global__") == len(gc.GRAD_KERNELS)
    assert set(re.findall(r"__global__[^{;]*?\b(?!__launch_bounds__)([A-Za-z]\w*)\s*\(", text)) == gc.GRAD_KERNELS
    assert all(name.startswith("ssqg_") for name in gc.GRAD_KERNELS)
    assert not re.findall(r"__global__[^{;]*?\b(k_\w+)\s*\(", text)
