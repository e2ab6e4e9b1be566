"""Thread schedules of the CPU emulation (tests/emu/hipemu.cpp): the kernels under adversarial, legal orders of their threads.

`lockstep`, the emulator's default, runs every thread of a workgroup in thread order between any two barriers and lets a
wave barrier order the whole workgroup: it cannot see a dependence between waves behind a wave barrier (ct::Fft's WAVE_LOCAL
instances stand on the promise that there is none), nor a read of a LOWER thread's LDS element behind no barrier.  The `waves`
schedules run one wavefront at a time through a whole workgroup-barrier interval, forward, reverse (waves last to first, lanes
63 to 0) and seeded (permutations redrawn every interval), on LDS that starts as NaN.

Three parts:
  1. the detector detects: six tiny kernels (tests/emu/selftest_kernels.cpp), wrong on purpose or correct, give a wrong or the
     right integer under exactly the schedules they should;
  2. every kernel of the product under five schedules: a race-free kernel cannot tell schedules apart (fixed summation orders,
     integer atomics only), so the output under every wave schedule is np.array_equal to the lockstep output, and the lockstep
     output is within the emulated modules' bounds of the oracle;
  3. the coverage gate: every __global__ kernel of pycwt_amd/csrc is launched by a case under `waves-reverse`, or is exempt
     because its body has no LDS, barrier or FFT (a schedule cannot matter to it).
None of this runs on a GPU, and nothing here provokes a fault: "fails" is a wrong integer in a buffer.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import pycwt_amd
from conftest import ROOT, load_golden, row_errors
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND as ADJOINT_BOUND, FORMS_OPTS, numpy_adjoint, random_g, rel
from test_kernels_emulated import grid
from test_power_emulated import power_bound

LOCKSTEP, WAVES, WAVES_REVERSE, WAVES_SEEDED = 0, 1, 2, 3
SCHEDULES = [("lockstep", LOCKSTEP, 0), ("waves", WAVES, 0), ("waves-reverse", WAVES_REVERSE, 0),
             ("waves-seeded:1", WAVES_SEEDED, 1), ("waves-seeded:2", WAVES_SEEDED, 2)]
ROW_BOUND = {64: 1e-11, 32: 5e-5}        # per row against orc.cwt_rows: the bound of test_kernels_randomized.py


@pytest.fixture()
def schedule(emu_library):
    """set(kind, seed) on the emulated library's process-global schedule; what was there before (lockstep, unless
    CWT_EMU_SCHEDULE says otherwise) is back when the test ends, however it ends."""
    dll = emu_library.dll
    dll.hipemu_launched.restype = C.c_size_t
    dll.hipemu_launched.argtypes = [C.c_char_p, C.c_size_t]
    kind, seed = C.c_int(0), C.c_uint(0)
    dll.hipemu_get_schedule(C.byref(kind), C.byref(seed))

    def set_schedule(k, s=0):
        assert dll.hipemu_set_schedule(int(k), C.c_uint(s)) == 0
    try:
        yield set_schedule
    finally:
        dll.hipemu_set_schedule(kind.value, seed)


def launched(lib):
    """the kernel names (template arguments dropped) launched since the last hipemu_clear_launched(), and the raw strings"""
    need = lib.dll.hipemu_launched(None, 0)
    buf = C.create_string_buffer(need)
    lib.dll.hipemu_launched(buf, need)
    raw = set(buf.value.decode().split("\n")) - {""}
    return {re.search(r"k_\w+", s).group(0) for s in raw}, raw


# ---- 1. the detector ------------------------------------------------------------------------------------------------------
SELFTESTS = {            # name: (id in hipemu_selftest, the element thread t reads)
    "cross_wave": (0, lambda t: t ^ 64),
    "cross_wave_ok": (1, lambda t: t ^ 64),
    "up": (2, lambda t: np.minimum(t + 1, 255)),
    "up_ok": (3, lambda t: (t & ~63) | ((t + 1) & 63)),
    "down": (4, lambda t: np.maximum(t - 1, 0)),
    "down_ok": (5, lambda t: (t & ~63) | ((t + 63) & 63)),
}
TEN_SEEDS = [("waves-seeded:%d" % s, WAVES_SEEDED, s) for s in range(1, 11)]
# whether the answer is right, per schedule, where the order decides it
EXPECT = {
    "cross_wave": {"lockstep": True, "waves": False, "waves-reverse": False},       # lockstep: the documented blind spot
    "up": {"lockstep": False, "waves": False, "waves-reverse": True},
    "down": {"lockstep": True, "waves": True, "waves-reverse": False},
}


def selftest(lib, which, blocks=3, salt=12345):
    out = np.full((blocks, 256), -7, dtype=np.int32)
    assert lib.dll.hipemu_selftest(SELFTESTS[which][0], blocks, salt, out.ctypes.data_as(C.c_void_p)) == 0
    t = np.arange(256)
    want = salt + 1000 * np.arange(blocks)[:, None] + SELFTESTS[which][1](t)[None, :]
    return bool(np.array_equal(out, want))


@pytest.mark.parametrize("which", ["cross_wave", "up", "down"])
def test_broken_kernels_fail_under_exactly_the_schedules_that_expose_them(emu_library, schedule, which):
    for label, kind, seed in SCHEDULES[:3]:
        schedule(kind, seed)
        assert selftest(emu_library, which) == EXPECT[which][label], (which, label)
    # a permutation of 4 waves x 64 lanes leaves every neighbour dependence intact with probability ~1 / 64!: every seed shows all three
    for label, kind, seed in TEN_SEEDS:
        schedule(kind, seed)
        assert not selftest(emu_library, which), (which, label)


@pytest.mark.parametrize("which", ["cross_wave_ok", "up_ok", "down_ok"])
def test_correct_kernels_pass_under_every_schedule(emu_library, schedule, which):
    for label, kind, seed in SCHEDULES[:3] + TEN_SEEDS:
        schedule(kind, seed)
        assert selftest(emu_library, which), (which, label)


def test_seeded_schedule_is_reproducible_and_unknown_kinds_are_refused(emu_library, schedule):
    """The same seed gives the same (wrong) integers whichever OS thread takes a workgroup; another seed gives others."""
    def wrong(seed):
        schedule(WAVES_SEEDED, seed)
        out = np.zeros((8, 256), dtype=np.int32)
        emu_library.dll.hipemu_selftest(4, 8, 0, out.ctypes.data_as(C.c_void_p))
        return out
    a, b, c = wrong(5), wrong(5), wrong(6)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert emu_library.dll.hipemu_set_schedule(4, 0) == -1 and emu_library.dll.hipemu_set_schedule(-1, 0) == -1
    kind, seed = C.c_int(0), C.c_uint(0)
    emu_library.dll.hipemu_get_schedule(C.byref(kind), C.byref(seed))
    assert (kind.value, seed.value) == (WAVES_SEEDED, 6)


# ---- 2. the product's kernels ---------------------------------------------------------------------------------------------
def types(prec):
    return (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)


class Buffers:
    """device buffers of a case, freed together with its plan"""
    def __init__(self, lib, plan):
        self.lib, self.plan, self.all = lib, plan, []

    def up(self, a):
        b = _hip.DeviceBuffer(a.nbytes, lib=self.lib)
        self.all.append(b)
        b.upload(self.plan, np.ascontiguousarray(a))
        return b

    def free(self):
        for b in self.all:
            b.free()
        self.plan.close()


def one_per_class(lib, N, prec, kind, param, sj, n0, opts, per=1, with_signal=True):
    """`per` scales of every row class of the grid (a class is a code path; the cases stay small)"""
    plan = _hip.Plan(N, prec, max_rows=len(sj), lib=lib, options=opts)
    classes = plan.classify(kind, param, 1.0, sj, n0, with_signal)
    plan.close()
    seen, keep = {}, []
    for i, c in enumerate(classes):
        seen[c] = seen.get(c, 0) + 1
        if seen[c] <= per:
            keep.append(i)
    return np.asarray(sj)[keep]


def rows_case(lib, prec, logn, n0_off, kind, param, rows, opts, need=(), with_signal=True, per=1, pad=0, sj=None, host=False,
              power=True):
    """One transform of a signal through the forms the options force: W (complex) and P (power) of the same plan, both into
    matrices with `pad` extra columns filled with a sentinel (power=False: W alone).  Lockstep check: W per row against the oracle, P against |W|^2,
    the padding untouched, the forms in `need` present.  A case that sets an accuracy target ("tolerance") is held to that target
    where it is looser than the round-off bound: it is what the plan was told to truncate at."""
    real, cplx = types(prec)
    bound = max(ROW_BOUND[prec], opts.get("tolerance", 0.0))
    N = 1 << logn
    n0 = N - n0_off
    m = orc.Mother(kind, param)
    opts = dict(opts)
    if sj is None:
        sj = one_per_class(lib, N, prec, kind, param, grid(n0, 1.0, m, rows), n0, opts, per, with_signal)
    x = np.random.default_rng(1000 * logn + prec).standard_normal(n0)
    nr, ld = len(sj), n0 + pad
    plan = _hip.Plan(N, prec, max_rows=nr, lib=lib, options=opts)
    if host:                                           # cwt_execute_host
        W, xhat = plan.execute_host(x, kind, param, 1.0, sj)
        outs = {"W": np.array(W), "xhat": np.array(xhat)}
        split, classes = plan.last_split(), plan.row_classes()
        plan.close()
    else:
        b = Buffers(lib, plan)
        try:
            xd, xh = b.up(x.astype(real)), b.up(np.zeros(N, dtype=cplx))
            Wd, Pd = b.up(np.full((nr, ld), -7 - 7j, dtype=cplx)), b.up(np.full((nr, ld), -7, dtype=real))
            if with_signal:
                plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, ld, n0)
                if power:
                    plan.transform_power(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Pd.ptr, ld, n0)
            else:
                plan.forward_fft(xd.ptr, n0, xh.ptr)
                plan.transform_rows(xh.ptr, kind, param, 1.0, sj, Wd.ptr, ld, n0)
                if power:
                    plan.transform_rows_power(xh.ptr, kind, param, 1.0, sj, Pd.ptr, ld, n0)
            split, classes = plan.last_split(), plan.row_classes()
            outs = {"W": Wd.download(plan, (nr, ld), cplx), "xhat": xh.download(plan, (N,), cplx)}
            if power:
                outs["P"] = Pd.download(plan, (nr, ld), real)
        finally:
            b.free()

    def verify():
        for form in need:
            assert split.get(form, 0) > 0 or any(c.startswith(form) for c in classes), (form, sorted(set(classes)), split)
        W = outs["W"][:, :n0]
        x64 = x.astype(real).astype(np.float64)
        ref = orc.cwt_rows(x64, 1.0, sj, m, N=N)[:, :n0]
        per_row, _ = row_errors(W, ref)
        assert per_row.max() < bound, (per_row.argmax(), per_row.max(), classes[per_row.argmax()])
        xref = np.fft.fft(x64, n=N)
        assert np.abs(outs["xhat"] - xref).max() < ROW_BOUND[prec] * np.abs(xref).max()
        if "P" in outs:
            power_bound(outs["P"][:, :n0], W, prec)
            assert np.all(outs["W"][:, n0:] == -7 - 7j) and np.all(outs["P"][:, n0:] == -7)
    return outs, verify


def batch_case(lib, prec, logn=15, nb=3, rows=40):
    """cwt_transform_batch / _batch_power: 3 signals with a padded leading dimension of x, W and P"""
    real, cplx = types(prec)
    N = 1 << logn
    n0, kind, param = N - 200, orc.MORLET, 6
    m = orc.Mother(kind, param)
    opts = {"ols_min_logn": 15, "poly_min_logn": 14, "aols_min_rows": 1}
    sj = one_per_class(lib, N, prec, kind, param, grid(n0, 1.0, m, rows), n0, opts)
    nr, x_ld, ld = len(sj), n0 + 5, n0 + 3
    X = np.full((nb, x_ld), np.nan)
    X[:, :n0] = np.random.default_rng(12).standard_normal((nb, n0))
    plan = _hip.Plan(N, prec, max_rows=nb * nr, lib=lib, options=opts)
    b = Buffers(lib, plan)
    try:
        xd, xh = b.up(X.astype(real)), b.up(np.zeros((nb, N), dtype=cplx))
        Wd, Pd = b.up(np.full((nb * nr, ld), -7 - 7j, dtype=cplx)), b.up(np.full((nb * nr, ld), -7, dtype=real))
        plan.transform_batch(xd.ptr, nb, x_ld, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, ld, n0)
        classes = plan.row_classes()
        plan.transform_batch_power(xd.ptr, nb, x_ld, n0, kind, param, 1.0, sj, xh.ptr, Pd.ptr, ld, n0)
        outs = {"W": Wd.download(plan, (nb, nr, ld), cplx), "P": Pd.download(plan, (nb, nr, ld), real)}
    finally:
        b.free()

    def verify():
        assert {"ols", "aols"} <= {c.split("/")[0] for c in classes}, sorted(set(classes))
        for s in range(nb):
            ref = orc.cwt_rows(X[s, :n0].astype(real).astype(np.float64), 1.0, sj, m, N=N)[:, :n0]
            per_row, _ = row_errors(outs["W"][s, :, :n0], ref)
            assert per_row.max() < ROW_BOUND[prec], (s, per_row.max(), classes[per_row.argmax()])
            power_bound(outs["P"][s, :, :n0], outs["W"][s, :, :n0], prec)
        assert np.all(outs["W"][:, :, n0:] == -7 - 7j) and np.all(outs["P"][:, :, n0:] == -7)
    return outs, verify


def adjoint_case(lib, prec, kind, param, adjoint_poly, rows=20, logn=15):
    """cwt_adjoint_rows on a batch of 2 with every stride padded (ldg > ncols, g_batch_ld > rows * ldg, xbar_ld > ncols): the
    padding of G holds NaN and must not be read, that of xbar holds 1e30 and must not be written.  Then accumulate = 1."""
    real, cplx = types(prec)
    N = 1 << logn
    n0 = N - 77
    m = orc.Mother(kind, param)
    opts = dict(FORMS_OPTS, adjoint_poly=adjoint_poly)
    sj = one_per_class(lib, N, prec, kind, param, grid(n0, 1.0, m, rows), n0, opts)
    nr, nb = len(sj), 2
    ldg, xbar_ld = n0 + 9, n0 + 4
    g_batch_ld = nr * ldg + 11
    rng = np.random.default_rng(3)
    G = random_g(rng, nb, nr, n0).astype(cplx)
    Gpad = np.full(nb * g_batch_ld, np.nan + 1j * np.nan, dtype=cplx)
    for s in range(nb):
        Gpad[s * g_batch_ld:s * g_batch_ld + nr * ldg].reshape(nr, ldg)[:, :n0] = G[s]
    base = rng.standard_normal((nb, n0)).astype(real)
    plan = _hip.Plan(N, prec, max_rows=nr, lib=lib, options=opts)
    classes = plan.classify(kind, param, 1.0, sj, n0, True)
    b = Buffers(lib, plan)
    try:
        Gd = b.up(Gpad)
        xb = b.up(np.full((nb, xbar_ld), 1e30, dtype=real))
        plan.adjoint_rows(Gd.ptr, nb, g_batch_ld, ldg, n0, kind, param, 1.0, sj, xb.ptr, xbar_ld, False)
        first = xb.download(plan, (nb, xbar_ld), real)
        acc0 = np.full((nb, xbar_ld), 1e30, dtype=real)
        acc0[:, :n0] = base
        xa = b.up(acc0)
        plan.adjoint_rows(Gd.ptr, nb, g_batch_ld, ldg, n0, kind, param, 1.0, sj, xa.ptr, xbar_ld, True)
        outs = {"xbar": first, "accumulated": xa.download(plan, (nb, xbar_ld), real), "G": Gd.download(plan, Gpad.shape, cplx)}
    finally:
        b.free()

    def verify():
        kinds = {c.split("/")[0] for c in classes}
        assert "poly" in kinds and len(kinds) >= 3, sorted(set(classes))
        assert np.all(outs["xbar"][:, n0:] == real(1e30)) and np.all(outs["accumulated"][:, n0:] == real(1e30))
        assert np.array_equal(outs["G"], Gpad, equal_nan=True)                   # (the input is not a scratch buffer either)
        for s in range(nb):
            ref = numpy_adjoint(G[s].astype(np.complex128), sj, m, N)
            assert rel(outs["xbar"][s, :n0], ref) <= ADJOINT_BOUND[prec], rel(outs["xbar"][s, :n0], ref)
        np.testing.assert_allclose(outs["accumulated"][:, :n0], base + outs["xbar"][:, :n0], rtol=0,
                                   atol=(1e-13 if prec == 64 else 1e-6) * np.abs(outs["xbar"][:, :n0]).max())
    return outs, verify


class TableMorlet:
    """A mother wavelet without device_id(): the shim computes its filter bank on the host (cwt_transform_rows_table)"""
    def __init__(self):
        self.m = pycwt_amd.Morlet(6)

    def psi_ft(self, f):
        return self.m.psi_ft(f)

    def flambda(self):
        return self.m.flambda()

    def coi(self):
        return self.m.coi()


def callers_case(lib, prec):
    """The callers' kernels through the Python shim on the series of the reference's fixture: wct (fft_rows, filter_rows, boxcar,
    products, coherence), xwt (cross spectrum), the device handles' reductions, icwt, the unpadded (Bluestein) transform and a
    filter bank of the caller's.  Lockstep check: the reference's values with the bounds of test_callers_emulated.py /
    test_shim_emulated.py (complex64: the row bound of this module in their place)."""
    from pycwt_amd import wavelet
    for p in wavelet._plans.values():                  # (a fresh plan per schedule: what a plan launches once is launched under each)
        p.close()
    wavelet._plans.clear()
    g = load_golden("callers")
    y1, y2, dt, dj = g["y1"], g["y2"], float(g["dt"]), float(g["dj"])
    m = pycwt_amd.Morlet(6)
    kw = dict(precision=prec)
    outs = {}
    outs["wct"], outs["awct"] = pycwt_amd.wct(y1, y2, dt, dj, -1, -1, False, 0.95, m, True, **kw)[:2]
    outs["xwt"] = pycwt_amd.xwt(y1, y2, dt, dj, -1, -1, 0.95, m, True, **kw)[0]
    W, sj = pycwt_amd.cwt(y1, dt, dj, -1, -1, m, **kw)[:2]
    outs["cwt"] = W
    outs["icwt"] = pycwt_amd.icwt(W, sj, dt, dj, m, **kw)
    T = pycwt_amd.cwt_device(y1, dt, dj, -1, -1, m, **kw)
    try:
        outs["global_power"], outs["scale_average"], outs["icwt_device"] = T.global_power(), T.scale_average(2.0, 8.0, dj), T.icwt(dj)
    finally:
        T.close()
    H = pycwt_amd.cwt_power_device(y1, dt, dj, -1, -1, m, **kw)
    try:
        outs["power"], outs["power_global"], outs["power_scale_average"] = H.power(), H.global_power(), H.scale_average(2.0, 8.0, dj)
    finally:
        H.close()
    outs["unpadded"] = pycwt_amd.cwt(y1, dt, dj, -1, -1, m, pad=False, **kw)[0]
    outs["unpadded_power"] = pycwt_amd.cwt_power(y1, dt, dj, -1, -1, m, pad=False, **kw)[0]
    outs["table"] = pycwt_amd.cwt(y1, dt, dj, -1, -1, TableMorlet(), **kw)[0]
    # boxcar windows on both sides of the ring kernel's limit, rows not a multiple of its strip
    rng = np.random.default_rng(4)
    real, cplx = types(prec)
    Tm = (rng.standard_normal((70, 300)) + 1j * rng.standard_normal((70, 300))).astype(cplx)
    wins = [rng.random(L) for L in (1, 3, 14, 17, 70)]
    plan = _hip.Plan(512, prec, max_rows=128, lib=lib)
    b = Buffers(lib, plan)
    try:
        a, o = b.up(Tm), b.up(np.zeros_like(Tm))
        for win in wins:
            plan.boxcar_scales(a.ptr, 70, 300, 300, win, o.ptr)
            outs["boxcar%d" % win.size] = o.download(plan, (70, 300), cplx)
    finally:
        b.free()

    def verify():
        from scipy.signal import convolve2d
        tight = prec == 64
        assert np.abs(outs["wct"] - g["wct"]).max() < (1e-10 if tight else 1e-3)
        assert np.abs(np.angle(np.exp(1j * (outs["awct"] - g["awct"])))).max() < 1e-9 or not tight
        tol = 1e-11 if tight else ROW_BOUND[32]
        assert np.abs(outs["xwt"] - g["xwt_W12"]).max() < tol * np.abs(g["xwt_W12"]).max()
        mo = orc.Mother(orc.MORLET, 6)
        ref = orc.cwt_rows(y1, dt, sj, mo, N=2 ** int(np.ceil(np.log2(y1.size))))[:, :y1.size]
        for key in ("cwt", "table"):
            assert row_errors(outs[key], ref)[0].max() < tol, key
        assert row_errors(outs["unpadded"], orc.cwt_rows(y1, dt, sj, mo, N=y1.size))[0].max() < tol
        power_bound(outs["unpadded_power"], outs["unpadded"], prec)
        power_bound(outs["power"], outs["cwt"], prec)
        P = np.abs(outs["cwt"].astype(np.complex128)) ** 2
        rt = 1e-11 if tight else 1e-4
        for key in ("global_power", "power_global"):
            np.testing.assert_allclose(outs[key], P.mean(axis=1), rtol=rt)
        w = np.where((sj >= 2.0) & (sj < 8.0), 1.0 / sj, 0.0)
        for key in ("scale_average", "power_scale_average"):
            np.testing.assert_allclose(outs[key], dj * dt / m.cdelta * (w[:, None] * P).sum(axis=0), rtol=rt, atol=1e-300)
        np.testing.assert_allclose(outs["icwt"], outs["icwt_device"], rtol=1e-10 if tight else 1e-3, atol=1e-11 if tight else 1e-3)
        for win in wins:
            want = convolve2d(Tm.astype(np.complex128), win[:, None], "same")
            np.testing.assert_allclose(outs["boxcar%d" % win.size], want, rtol=0, atol=(1e-12 if tight else 2e-5) * win.size)
    return outs, verify


def monte_carlo_case(lib, prec):
    """k_normal_fill, k_ar1_filter, k_coherence_hist (LDS histogram with integer atomics) and the spectrum range of the
    automatic tolerance (two tree reductions in LDS): against numpy / scipy."""
    outs = {}
    kw = dict(dt=1.0, dj=0.5, s0=2.0, J=6, mc_count=3, progress=False, wavelet="morlet", cache=False, precision=prec)
    outs["sig_ar1"] = pycwt_amd.wct_significance(0.6, 0.8, rng="device", seed=11, surrogates="ar1", **kw)
    real, cplx = types(prec)
    rng = np.random.default_rng(11)
    r2 = rng.random((5, 3000)).astype(real)
    r2[0, ::7], r2[1, ::5], r2[2, ::3] = np.nan, 1.0, -0.25
    lo, hi = np.array([0, 100, 1499, 2999, 7], dtype=np.int64), np.array([3000, 2900, 1500, 2999, 8], dtype=np.int64)
    spec = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(cplx)
    plan = _hip.Plan(4096, prec, max_rows=8, lib=lib)
    b = Buffers(lib, plan)
    try:
        rd, ld_, hd, hist = b.up(r2), b.up(lo), b.up(hi), b.up(np.zeros((5, 1000), dtype=np.uint64))
        plan.coherence_histogram(rd.ptr, 3000, 5, ld_.ptr, hd.ptr, 3000, 1000, hist.ptr)
        outs["hist"] = hist.download(plan, (5, 1000), np.uint64)
        sd = b.up(spec)
        outs["range"] = np.array(plan.spectrum_range(sd.ptr, 5000))
        e, y = b.up(np.zeros(5000, dtype=real)), b.up(np.zeros(4000, dtype=real))
        plan.random_normal(2024, 3, 5000, 1.5, e.ptr)
        plan.ar1_filter(e.ptr, 1000, 4000, 0.7, y.ptr)
        outs["normal"], outs["ar1"] = e.download(plan, (5000,), real), y.download(plan, (4000,), real)
    finally:
        b.free()

    def verify():
        from scipy.signal import lfilter
        want = np.zeros((5, 1000), dtype=np.uint64)
        for s in range(5):
            with np.errstate(invalid="ignore"):
                v = np.floor(r2[s, lo[s]:hi[s]] * real(1000))
            want[s] = np.bincount(v[(v >= 0) & (v < 1000)].astype(int), minlength=1000)
        np.testing.assert_array_equal(outs["hist"], want)
        a2 = np.abs(spec.astype(np.complex128)) ** 2
        np.testing.assert_allclose(outs["range"][:2], [np.sqrt(a2.max()), np.sqrt(a2.mean())], rtol=1e-12)
        z = outs["normal"].astype(np.float64) / 1.5
        assert abs(z.mean()) < 0.06 and abs(z.std() - 1) < 0.05                    # 5000 draws: 4 sigma of either statistic
        ref = lfilter([1, 0], [1, -0.7], outs["normal"].astype(np.float64))[1000:]
        np.testing.assert_allclose(outs["ar1"], ref, rtol=0, atol=(1e-12 if prec == 64 else 1e-5) * np.abs(ref).max())
        sig = outs["sig_ar1"]
        ok = np.isfinite(sig)
        assert ok.any() and (sig[ok] > 0).all() and (sig[ok] <= 1).all()
    return outs, verify


TWO_PASS_OPTS = [            # the generic (run-time geometry) kernels: every tile size 2^8 ... 2^13
    (8, {"lmax": 16, "wg_points": 256, "narrow_max_k": 16}),
    (12, {"lmax": 64, "wg_points": 256, "chunk_rows": 3}),
    (12, {"lmax": 64, "wg_points": 512, "chunk_rows": 1}),
    (12, {"lmax": 64, "narrow": 0, "wg_points": 1024}),
    (12, {"lmax": 128, "wg_points": 2048, "narrow_max_k": 256}),
    (13, {"lmax": 128, "wg_points": 4096, "narrow": 0}),
    (14, {"lmax": 128, "wg_points": 8192}),
]
OLS = {"ols_min_logn": 15, "poly": 0, "aols_min_rows": 1}
POLY = {"poly_min_logn": 14, "ols": 0}
MORLET6 = orc.Mother(orc.MORLET, 6)

CASES = {}
for _logn in range(3, 13):          # single-workgroup lengths: k_direct / k_small, REM = 0 ... 3, the WAVE plane instances
    CASES["single_wg_2^%d" % _logn] = lambda lib, prec, L=_logn: rows_case(
        lib, prec, L, (1 << L) // 10, orc.MORLET, 6, 7, {}, need=("small",), host=L % 2 == 0, sj=grid(1 << L, 1.0, MORLET6, 7))
for _i, (_logn, _o) in enumerate(TWO_PASS_OPTS):
    CASES["generic_geometry_%d" % _i] = lambda lib, prec, L=_logn, o=_o, i=_i: rows_case(
        lib, prec, L, 5, [orc.MORLET, orc.DOG, orc.PAUL][i % 3], [6, 2, 4][i % 3], 12, o, per=2, power=i in (0, 3, 6))
CASES["two_pass_ct_2^13"] = lambda lib, prec: rows_case(lib, prec, 13, 192, orc.MORLET, 6, 16, {"narrow_terms": 1},
                                                         need=("two_pass", "narrow"), pad=3)
CASES["two_pass_ct_2^15"] = lambda lib, prec: rows_case(lib, prec, 15, 9, orc.DOG, 2, 12, {"ols": 0, "poly": 0}, need=("two_pass",))
CASES["two_pass_ct_rows_2^15"] = lambda lib, prec: rows_case(lib, prec, 15, 9, orc.MORLET, 6, 12, {"ols": 0, "poly": 0, "band_pass_a": 0},
                                                              need=("two_pass",), with_signal=False, power=False)
for _t in (1, 2, 3, 4):             # logK 10, 1 ... 4 aliased terms
    CASES["narrow_terms_%d" % _t] = lambda lib, prec, t=_t: rows_case(lib, prec, 14, 383, [orc.MORLET, orc.DOG][t % 2], [6, 2][t % 2], 14,
                                                                      {"narrow_terms": t, "narrow_big": 0}, need=("narrow",), power=t in (1, 4))
CASES["narrow_many"] = lambda lib, prec: rows_case(
    lib, prec, 15, 0, orc.MORLET, 6, 0, {"narrow_terms": 16, "narrow_big": 0, "ols": 0, "poly": 0}, need=("narrow_many",),
    sj=2.9 * (1 << 15) / np.array([5000.0, 7000.0, 9000.0, 12500.0, 15500.0]))
CASES["narrow_k2048"] = lambda lib, prec: rows_case(
    lib, prec, 15, 0, orc.DOG, 2, 0, {"narrow_big": 1, "big_terms": 8, "narrow_terms": 1, "ols": 0, "poly": 0},
    need=("narrow_k2048",) if prec == 64 else (), sj=2.5 * (1 << 15) / np.array([1500.0, 3000.0, 6000.0, 7900.0, 12000.0]))
CASES["poly_morlet"] = lambda lib, prec: rows_case(lib, prec, 15, 37, orc.MORLET, 6, 64, POLY, need=("poly",), pad=13)
CASES["poly_dog_chunks_spectrum_only"] = lambda lib, prec: rows_case(lib, prec, 15, 100, orc.DOG, 2, 48, dict(POLY, poly_chunk_mb=1),
                                                                       need=("poly",), with_signal=False, per=3)
CASES["poly_low_degree_taylor"] = lambda lib, prec: rows_case(lib, prec, 15, 321, orc.MORLET, 6, 64,
                                                              dict(POLY, poly_cheb=0, tolerance=1e-9 if prec == 64 else 3e-5), need=("poly",))
CASES["ols_morlet"] = lambda lib, prec: rows_case(lib, prec, 15, 77, orc.MORLET, 6, 48, OLS, need=("ols", "aols"), pad=13)
CASES["ols_dog_nyquist_rows"] = lambda lib, prec: rows_case(lib, prec, 15, 0, orc.DOG, 2, 48, OLS, need=("ols", "aols"))
CASES["ols_dog_odd_order"] = lambda lib, prec: rows_case(lib, prec, 15, 7, orc.DOG, 3, 48, dict(OLS, ols_big=0), need=("aols",))
CASES["ols_paul"] = lambda lib, prec: rows_case(lib, prec, 15, 77, orc.PAUL, 4, 96, OLS, need=("aols",) if prec == 32 else ())
# blocks of two tiles: opt-in at complex128; complex64 (pairs of blocks in packed registers) takes them from 2^17 on
CASES["ols_double_blocks"] = lambda lib, prec: rows_case(
    lib, prec, 16 if prec == 64 else 17, 2900, orc.MORLET if prec == 64 else orc.PAUL, 6 if prec == 64 else 4, 72,
    dict(OLS, ols_big=1, ols_big_min_halo=256 if prec == 64 else 512), need=("ols2/", "ols/"), power=prec == 64)
CASES["batch_of_3_padded"] = batch_case
for _ap in (1, 0):
    CASES["adjoint_morlet_poly%d" % _ap] = lambda lib, prec, ap=_ap: adjoint_case(lib, prec, orc.MORLET, 6, ap, logn=14 + ap)
CASES["adjoint_dog"] = lambda lib, prec: adjoint_case(lib, prec, orc.DOG, 2, 1, logn=14)
CASES["callers"] = callers_case
CASES["monte_carlo"] = monte_carlo_case
# interval coefficients on the 8192- and 16384-point tiles (k_poly_coef<T, 13 | 14>): K' = N / 64 of that size, complex128 only
# (complex64 keeps intervals of 128 samples: the same instantiation at twice the length)
CASES_ONE_PRECISION = {
    "poly_coef_tile_2^13": (64, lambda lib, prec: rows_case(lib, prec, 19, 77, orc.MORLET, 6, 0, {}, need=("poly/K8192",), with_signal=False,
                                                            sj=np.array([150.0, 260.0]), power=False)),
    "poly_coef_tile_2^14": (64, lambda lib, prec: rows_case(lib, prec, 20, 77, orc.MORLET, 6, 0, {}, need=("poly/K16384",), with_signal=False,
                                                            sj=np.array([230.0]), power=False)),
}
ALL_CASES = [(name, prec) for name in CASES for prec in (64, 32)] + [(name, p) for name, (p, _) in CASES_ONE_PRECISION.items()]

LAUNCHED = {}            # (case, precision) -> (names, raw strings) launched under waves-reverse


def run_case(lib, schedule, name, prec, labels):
    """outputs of the case under the schedules named; fills LAUNCHED from the waves-reverse run"""
    fn = CASES[name] if name in CASES else CASES_ONE_PRECISION[name][1]
    got = {}
    for label, kind, seed in SCHEDULES:
        if label not in labels:
            continue
        schedule(kind, seed)
        lib.dll.hipemu_clear_launched()
        got[label] = fn(lib, prec)
        if label == "waves-reverse":
            LAUNCHED[name, prec] = launched(lib)
    return got


@pytest.mark.parametrize("name,prec", ALL_CASES, ids=["%s-fp%d" % c for c in ALL_CASES])
def test_wave_schedules_give_the_bits_of_lockstep(emulated, schedule, name, prec):
    got = run_case(emulated, schedule, name, prec, [s[0] for s in SCHEDULES])
    base, verify = got["lockstep"]
    verify()
    for label, (outs, _) in got.items():
        assert outs.keys() == base.keys()
        for key, a in base.items():
            assert np.array_equal(np.asarray(outs[key]), np.asarray(a), equal_nan=True), (name, prec, label, key)


# ---- 3. the coverage gate -------------------------------------------------------------------------------------------------
EXEMPT = {              # no LDS, no __syncthreads(), no ct::Fft in the body: a schedule cannot matter
    "k_queue_probe_wait": "one thread polling a flag in global memory (and compiled for the device only)",
    "k_queue_probe_set": "one thread, one global atomic store (and compiled for the device only)",
}


def kernels_of_the_product():
    """name -> body text of every __global__ kernel in pycwt_amd/csrc/*.hpp and abi.hip"""
    found = {}
    csrc = os.path.join(ROOT, "pycwt_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hpp"))) + [os.path.join(csrc, "abi.hip")]:
        text = open(path).read()
        for mt in re.finditer(r"__global__[^{;]*?\b(k_\w+)\s*\(", text):
            start = i = text.index("{", mt.end())
            depth = 0
            while True:
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
                if depth == 0:
                    break
            found[mt.group(1)] = text[start:i]
    return found


def test_every_kernel_is_launched_under_the_reverse_wave_schedule(emulated, schedule):
    for name, prec in ALL_CASES:                       # (cases the parametrised test has not run in this process: run them now)
        if (name, prec) not in LAUNCHED:
            run_case(emulated, schedule, name, prec, ["waves-reverse"])
    names = set().union(*(v[0] for v in LAUNCHED.values()))
    raw = set().union(*(v[1] for v in LAUNCHED.values()))
    kernels = kernels_of_the_product()
    assert len(kernels) >= 45, sorted(kernels)
    for k, reason in EXEMPT.items():
        assert reason and not re.search(r"HIP_DYNAMIC_SHARED|__shared__|__syncthreads|wave_sync|Fft|_body\s*[<(]", kernels[k]), k
    missing = sorted(set(kernels) - names - set(EXEMPT))
    assert not missing, missing
    for tile in (12, 13, 14):                          # the three tile sizes of the interval coefficients are three instantiations
        assert any(re.search(r"k_poly_coef<T, %d\b" % tile, s) for s in raw), (tile, sorted(raw))
