"""The kernels of cwt_icwt_shrink_adjoint under the wavefront schedules of the CPU emulation (tests/emu/hipemu.cpp), in the manner of
tests/test_shrink_schedules_emulated.py: forward, reverse and seeded wave orders give the bits of the lockstep order -- the LDS tree
of shgrad_rows is the thing under test.  The kernels of cwt_kernels_shrink_grad.hpp are called shgrad_* and are gated here: each of
them is launched under every schedule, and the set of names is read from the header."""
import numpy as np
import pytest

import shrink_grad_common as gc
from test_emu_schedules import LOCKSTEP, SCHEDULES, schedule  # noqa: F401  (the fixture that sets and restores the schedule)

WAVE_SCHEDULES = [s for s in SCHEDULES if s[1] != LOCKSTEP]


@pytest.mark.parametrize("prec", gc.PRECS)
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, prec):
    schedule(LOCKSTEP)
    base = gc.schedule_case(emu_library, prec)
    for label, kind, seed in WAVE_SCHEDULES:
        schedule(kind, seed)
        emu_library.dll.hipemu_clear_launched()
        got = gc.schedule_case(emu_library, prec)
        log = gc.launch_log(emu_library)
        assert all(any(name in s for s in log) for name in gc.KERNELS), (label, log)
        assert np.array_equal(base, got), label


@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("mode", gc.MODES)
def test_closed_form_under_every_schedule(emu_library, schedule, prec, mode):
    """the export cases that cross a slice (rows 1 and 9 x columns 2049 and 4099), against the closed form under each schedule"""
    for label, kind, seed in WAVE_SCHEDULES:
        schedule(kind, seed)
        with gc.Dev(emu_library, 16, prec, max_rows=16) as dev:
            for nrows in (1, 9):
                for ncols in (2049, 4099):
                    gc.check_closed_form(dev, nrows, ncols, "mixed", mode)


def test_every_kernel_is_known_to_the_schedule_test():
    """the kernels of the header are exactly those the schedule test launches, and none of them is named k_* (those are gated by
    tests/test_emu_schedules.py, whose cases do not launch them)"""
    names, k_names = gc.kernels_of_the_header()
    assert names == gc.KERNELS and not k_names
