"""The kernels of the synchrosqueezed transform under the wavefront schedules of the CPU emulation (tests/emu/hipemu.cpp), in the
manner of tests/test_emu_schedules.py: forward, reverse and seeded wave orders give the bits of the lockstep order.  That module's
coverage gate lists the kernels named k_*; the kernels of cwt_kernels_ssq.hpp are called ssq_* and are gated here: each of them is
launched under every schedule, and the set of names is read from the header."""
import os
import re

import numpy as np
import pytest

import ssq_common as sc
from conftest import ROOT
from test_emu_schedules import LOCKSTEP, SCHEDULES, schedule  # noqa: F401  (the fixture that sets and restores the schedule)

SSQ_KERNELS = {"ssq_spec_deriv", "ssq_zero", "ssq_reassign"}
WAVE_SCHEDULES = [s for s in SCHEDULES if s[1] != LOCKSTEP]


def schedule_case(lib, prec):
    """the derivative of a spectrum out of place and in place; a reassignment of 13 x 1000 entries in two row chunks (a first call
    that zero-fills, a second that accumulates), into a padded T: every kernel, as bytes"""
    with sc.Dev(lib, 4096, prec, max_rows=16) as dev:
        rng = np.random.default_rng(8)
        x = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(dev.cplx)
        xd, yd = dev.up(x), dev.up(np.zeros(4096, dtype=dev.cplx))
        dev.plan.spectrum_derivative(xd.ptr, 0.5, yd.ptr)
        dev.plan.spectrum_derivative(xd.ptr, 0.5, xd.ptr)
        y, y2 = yd.download(dev.plan, (4096,), dev.cplx), xd.download(dev.plan, (4096,), dev.cplx)
        dev.release()
        W, dW, w, _ = sc.synthetic(21, 13, 1000, 5, prec)
        T = sc.run_reassign(dev, W, dW, w, 5, chunks=8)
    return np.concatenate([y.view(np.uint8), y2.view(np.uint8), T.view(np.uint8).ravel()])


@pytest.mark.parametrize("prec", sc.PRECS)
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, prec):
    schedule(LOCKSTEP)
    base = schedule_case(emu_library, prec)
    for label, kind, seed in WAVE_SCHEDULES:
        schedule(kind, seed)
        emu_library.dll.hipemu_clear_launched()
        got = schedule_case(emu_library, prec)
        log = sc.launch_log(emu_library)
        assert all(any(name in s for s in log) for name in SSQ_KERNELS), (label, log)
        assert np.array_equal(base, got), label


def test_every_ssq_kernel_is_known_to_the_schedule_test():
    """the kernels of cwt_kernels_ssq.hpp are exactly those the schedule test launches, and none of them is named k_* (those are
    gated by tests/test_emu_schedules.py, whose cases do not launch them)"""
    text = open(os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_ssq.hpp")).read()
    assert set(re.findall(r"__global__[^{;]*?\b(ssq_\w+)\s*\(", text)) == SSQ_KERNELS
    assert not re.findall(r"__global__[^{;]*?\b(k_\w+)\s*\(", text)
