"""SURVEY.md 5 / VERDICT r05 7: the host logic (plan_host.cpp: the index arithmetic that sizes every launch and scratch buffer)
and the kernels' own indexing on the CPU stand-in, under -fsanitize=address,undefined.

The instrumented build of the unmodified sources takes ~6 minutes and the two kernel suites ~6 more, so this runs when asked
for: CWT_RUN_SANITIZERS=1 python -m pytest tests/test_sanitizers.py   (once per round; the record of the last run is
profiles/r06_sanitizer.txt).

The same kind of opt-in rerun for the emulator's thread schedules: CWT_RUN_SCHEDULES=1 python -m pytest tests/test_sanitizers.py -s
(record: profiles/emu_schedules.txt)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("CWT_RUN_SANITIZERS"), reason="set CWT_RUN_SANITIZERS=1 (12 minutes: instrumented build + two kernel suites)")
def test_kernel_suites_under_address_and_undefined_behaviour_sanitizers():
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import build_emu
    build_emu.build(asan=True)
    env = build_emu.sanitizer_env()
    env["PYTHONPATH"] = ROOT
    env.pop("CWT_RUN_SANITIZERS", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_kernels_randomized.py", "tests/test_new_forms_emulated.py",
                        "tests/test_c_host.py", "tests/test_exports_edges.py", "-x", "-q", "-n", "6", "-m", "not gpu"], cwd=ROOT, env=env, capture_output=True, text=True)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "ERROR: AddressSanitizer" not in tail and "runtime error:" not in tail, tail


SCHEDULE_MODULES = ["tests/test_kernels_emulated.py", "tests/test_kernels_randomized.py", "tests/test_new_forms_emulated.py",
                    "tests/test_power_emulated.py", "tests/test_adjoint_emulated.py", "tests/test_callers_emulated.py",
                    "tests/test_exports_edges.py"]


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("CWT_RUN_SCHEDULES"), reason="set CWT_RUN_SCHEDULES=1 (the seven emulated kernel modules, twice)")
@pytest.mark.parametrize("sched", ["waves-reverse", "waves-seeded:1"])
def test_emulated_kernel_modules_under_a_wave_schedule(sched):
    """The emulated kernel modules as they are, in a child process whose emulator runs one wavefront at a time (CWT_EMU_SCHEDULE,
    tests/emu/hipemu.cpp): a dependence between waves behind a wave barrier, or between lanes behind none, fails a module's own
    assertions.  tests/test_emu_schedules.py is the always-on part; the record of the last run is profiles/emu_schedules.txt."""
    import time
    env = dict(os.environ, PYTHONPATH=ROOT, CWT_EMU_SCHEDULE=sched)
    env.pop("CWT_RUN_SCHEDULES", None)
    cmd = [sys.executable, "-m", "pytest"] + SCHEDULE_MODULES + ["-q", "-n", "6", "-m", "not gpu", "-p", "no:cacheprovider"]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    tail = (r.stdout + r.stderr)[-4000:]
    print("CWT_EMU_SCHEDULE=%s %s\n  -> exit %d, %.0f s: %s" % (sched, " ".join(cmd[1:]), r.returncode, time.time() - t0,
                                                              tail.strip().splitlines()[-1] if tail.strip() else ""))
    assert r.returncode == 0, tail
