"""The weighted output (G = (alpha Q) W written by the row kernels: cwt_transform_weighted, cwt_transform_batch_weighted) on the
CPU emulation of the HIP runtime (tests/emu).

Every row form is forced with the options of test_power_emulated.FORMS, and the weighted output of a plan is compared with
alpha * Q * W of the complex output of the SAME plan, real and imaginary parts separately, under the rule of that module's
power_bound: per row max|dG| / max|reference| <= 32 eps of the precision, NaN where the reference is NaN.  (The kernel rounds
t = alpha q and t re, t im: two roundings per part; the reference is formed in float64 from the plan's W.)  Then the strides
(padding columns and rows not asked for keep a sentinel, Q is not written), the batch call, what is refused, and the
wavefront schedules of the emulator.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_kernels_emulated import grid
from test_power_emulated import EPS32, FORMS, types

SENTINEL = -7.0
ALPHAS = [2.0, -0.75]


def draw_q(seed, shape, real):
    """seeded normal weights, both signs, about 1 % exact zeros"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal(shape)
    Q[rng.random(shape) < 0.01] = 0.0
    return Q.astype(real)


def weighted_bound(G, W, Q, alpha, prec):
    """per row and per part max|G - alpha Q W| / max|alpha Q W| <= 32 eps, NaN positions identical"""
    ref = alpha * np.asarray(Q, dtype=np.float64) * np.asarray(W).astype(np.complex128)
    G = np.asarray(G).astype(np.complex128)
    assert G.shape == ref.shape
    worst = 0.0
    for got, want in ((G.real, ref.real), (G.imag, ref.imag)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        d = np.where(ok, np.abs(got - want), 0.0).max(axis=-1)
        peak = np.where(ok, np.abs(want), 0.0).max(axis=-1)
        err = d / np.where(peak == 0, 1.0, peak)
        assert err.max() <= EPS32[prec], (err.max(), EPS32[prec])
        worst = max(worst, err.max())
    return worst


def outputs(lib, N, x, kind, param, sj, prec, opts, alphas=ALPHAS, ld_pad=0, extra_rows=0, seed=21):
    """W, Q, {alpha: G}, split of one plan: cwt_transform, then cwt_transform_weighted per alpha into an
    (rows + extra_rows) x (n0 + ld_pad) matrix prefilled with SENTINEL (returned whole, as Q is after the calls)."""
    real, cplx = types(prec)
    n0, rows = x.size, len(sj)
    ld, nr = n0 + ld_pad, rows + extra_rows
    Q = draw_q(seed, (nr, ld), real)
    plan = _hip.Plan(N, prec, max_rows=rows, lib=lib, options=opts)
    bufs = []

    def up(a):
        b = _hip.DeviceBuffer(a.nbytes, lib=lib)
        bufs.append(b)
        b.upload(plan, np.ascontiguousarray(a))
        return b
    try:
        xd, xh, Wd, Qd = up(x.astype(real)), up(np.zeros(N, dtype=cplx)), up(np.zeros((rows, n0), dtype=cplx)), up(Q)
        plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        split = plan.last_split()
        W = Wd.download(plan, (rows, n0), cplx)
        G = {}
        for alpha in alphas:
            Gd = up(np.full((nr, ld), SENTINEL * (1 + 1j), dtype=cplx))
            plan.transform_weighted(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Qd.ptr, alpha, Gd.ptr, ld, n0)
            assert plan.last_split() == split          # the same row table, the same forms
            G[alpha] = Gd.download(plan, (nr, ld), cplx)
        Q_after = Qd.download(plan, (nr, ld), real)
    finally:
        for b in bufs:
            b.free()
        plan.close()
    assert np.array_equal(Q_after.view(np.uint8), Q.view(np.uint8))          # Q is never written
    return W, Q, G, split


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", FORMS, ids=[f[0] for f in FORMS])
def test_every_row_form_weighted_equals_alpha_q_w_of_the_same_plan(emu_library, prec, name, N, n0, kind, param, rows, opts, form):
    x = np.random.default_rng(7).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    W, Q, G, split = outputs(emu_library, N, x, kind, param, sj, prec, opts)
    form = form[prec] if isinstance(form, dict) else form
    assert split[form] > 0, split
    for alpha in ALPHAS:
        weighted_bound(G[alpha], W, Q, alpha, prec)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", [FORMS[1], FORMS[4], FORMS[6], FORMS[9]],
                         ids=["single_wg", "ols", "aols", "poly"])
def test_strides_leave_padding_other_rows_and_q_alone(emu_library, prec, name, N, n0, kind, param, rows, opts, form):
    real, cplx = types(prec)
    x = np.random.default_rng(9).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    W, Q, G, _ = outputs(emu_library, N, x, kind, param, sj, prec, opts, alphas=[2.0], ld_pad=5, extra_rows=2)
    G = G[2.0]
    sentinel = np.full(1, SENTINEL * (1 + 1j), dtype=cplx).view(np.uint8)
    pad = np.ascontiguousarray(G[:len(sj), n0:]).view(np.uint8).reshape(-1, sentinel.size)
    extra = np.ascontiguousarray(G[len(sj):]).view(np.uint8).reshape(-1, sentinel.size)
    assert np.all(pad == sentinel) and np.all(extra == sentinel)              # the sentinel's bits
    weighted_bound(G[:len(sj), :n0], W, Q[:len(sj), :n0], 2.0, prec)


@pytest.mark.parametrize("prec,kind,param", [(64, orc.MORLET, 6), (32, orc.DOG, 2), (64, orc.PAUL, 4)])
def test_batch_weighted(emu_library, prec, kind, param):
    """cwt_transform_batch_weighted against alpha Q W of cwt_transform_batch: the shapes of test_batch_power"""
    real, cplx = types(prec)
    es = np.dtype(real).itemsize
    lib = emu_library
    N, nb = 1 << 15, 3
    n0 = N - 200
    X = np.random.default_rng(12).standard_normal((nb, n0))
    sj = grid(n0, 1.0, orc.Mother(kind, param), 24)
    rows = len(sj)
    Q = draw_q(22, (nb * rows, n0), real)
    plan = _hip.Plan(N, prec, max_rows=nb * rows, lib=lib, options={"ols_min_logn": 15, "poly_min_logn": 14})
    xd, xh = _hip.DeviceBuffer(nb * n0 * es, lib=lib), _hip.DeviceBuffer(nb * N * 2 * es, lib=lib)
    Wd, Gd = _hip.DeviceBuffer(nb * rows * n0 * 2 * es, lib=lib), _hip.DeviceBuffer(nb * rows * n0 * 2 * es, lib=lib)
    Qd = _hip.DeviceBuffer(nb * rows * n0 * es, lib=lib)
    try:
        xd.upload(plan, X.astype(real))
        Qd.upload(plan, Q)
        plan.transform_batch(xd.ptr, nb, n0, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        split = plan.last_split()
        W = Wd.download(plan, (nb * rows, n0), cplx)
        for alpha in ALPHAS:
            plan.transform_batch_weighted(xd.ptr, nb, n0, n0, kind, param, 1.0, sj, xh.ptr, Qd.ptr, alpha, Gd.ptr, n0, n0)
            assert plan.last_split() == split
            weighted_bound(Gd.download(plan, (nb * rows, n0), cplx), W, Q, alpha, prec)
        assert np.array_equal(Qd.download(plan, (nb * rows, n0), real), Q)
    finally:
        for b in (xd, xh, Wd, Gd, Qd):
            b.free()
        plan.close()


def test_entry_points_and_refusals(emu_library):
    """No weighted export from a spectrum alone (the binding says so); Q aliasing G, ld < ncols and NULL pointers are refused
    with the usual status and a message."""
    lib = emu_library
    assert not hasattr(lib.dll, "cwt_transform_rows_weighted")
    n0, N = 200, 256
    sj = np.array([2.0, 4.0, 8.0])
    plan = _hip.Plan(N, 64, max_rows=8, lib=lib)
    xd, xh = _hip.DeviceBuffer(n0 * 8, lib=lib), _hip.DeviceBuffer(N * 16, lib=lib)
    Gd, Qd = _hip.DeviceBuffer(3 * n0 * 16, lib=lib), _hip.DeviceBuffer(3 * n0 * 8, lib=lib)
    try:
        xd.upload(plan, np.random.default_rng(1).standard_normal(n0))
        Qd.upload(plan, np.ones((3, n0)))
        with pytest.raises(NotImplementedError, match="spectrum"):
            plan.transform_rows_weighted(xh.ptr, orc.MORLET, 6.0, 1.0, sj, Qd.ptr, 2.0, Gd.ptr, n0, n0)
        with pytest.raises(_hip.HipError, match="overlap"):                    # Q inside G
            plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Gd.ptr, 2.0, Gd.ptr, n0, n0)
        with pytest.raises(_hip.HipError, match="overlap"):                    # ... and its last element on G's first
            plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Gd.ptr - (3 * n0 - 1) * 8, 2.0, Gd.ptr, n0, n0)
        with pytest.raises(_hip.HipError, match="ncols"):
            plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Qd.ptr, 2.0, Gd.ptr, n0 - 1, n0)
        with pytest.raises(_hip.HipError, match="NULL"):
            plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, 0, 2.0, Gd.ptr, n0, n0)
        with pytest.raises(_hip.HipError, match="NULL"):
            plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Qd.ptr, 2.0, 0, n0, n0)
        with pytest.raises(_hip.HipError, match="overlap"):
            plan.transform_batch_weighted(xd.ptr, 1, n0, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Gd.ptr + 16, 2.0, Gd.ptr, n0, n0)
        with pytest.raises(_hip.HipError, match="ncols"):
            plan.transform_batch_weighted(xd.ptr, 1, n0, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Qd.ptr, 2.0, Gd.ptr, n0 - 1, n0)
        # a refused call leaves no state: the next transform is the plain one
        Wd = _hip.DeviceBuffer(3 * n0 * 16, lib=lib)
        plan.transform(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        plan.transform_weighted(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Qd.ptr, 1.0, Gd.ptr, n0, n0)
        assert np.array_equal(Wd.download(plan, (3, n0), np.complex128), Gd.download(plan, (3, n0), np.complex128))
        Wd.free()
    finally:
        for b in (xd, xh, Gd, Qd):
            b.free()
        plan.close()


# ---- wavefront schedules (tests/emu/hipemu.cpp), as tests/test_emu_schedules.py runs them ------------------------------------
LOCKSTEP, WAVES, WAVES_REVERSE, WAVES_SEEDED = 0, 1, 2, 3
WAVE_SCHEDULES = [("waves", WAVES, 0), ("waves-reverse", WAVES_REVERSE, 0), ("waves-seeded:1", WAVES_SEEDED, 1)]


@pytest.fixture()
def schedule(emu_library):
    dll = emu_library.dll
    kind, seed = C.c_int(0), C.c_uint(0)
    dll.hipemu_get_schedule(C.byref(kind), C.byref(seed))

    def set_schedule(k, s=0):
        assert dll.hipemu_set_schedule(int(k), C.c_uint(s)) == 0
    try:
        yield set_schedule
    finally:
        dll.hipemu_set_schedule(kind.value, seed)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", [FORMS[4], FORMS[5], FORMS[9]], ids=["ols", "aols_paul", "poly"])
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, prec, name, N, n0, kind, param, rows,
                                                               opts, form):
    """A race-free kernel cannot tell legal thread orders apart: forward, reverse and seeded wavefront orders on NaN-filled
    LDS give the weighted output of the lockstep order bit for bit."""
    x = np.random.default_rng(7).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    schedule(LOCKSTEP)
    W, Q, G0, split = outputs(emu_library, N, x, kind, param, sj, prec, opts, alphas=[2.0])
    form = form[prec] if isinstance(form, dict) else form
    assert split[form] > 0, split
    weighted_bound(G0[2.0], W, Q, 2.0, prec)
    for label, k, s in WAVE_SCHEDULES:
        schedule(k, s)
        _, _, G, split_s = outputs(emu_library, N, x, kind, param, sj, prec, opts, alphas=[2.0])
        assert split_s == split
        assert np.array_equal(G[2.0].view(np.uint8), G0[2.0].view(np.uint8)), label
