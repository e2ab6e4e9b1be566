"""The power output (|W|^2 written by the row kernels: cwt_transform_power and its siblings, cwt_power*) on the CPU emulation
of the HIP runtime (tests/emu).

Every row form is forced with the plan options the other emulated tests use, and the power of a plan is compared with
re^2 + im^2 of the complex output of the SAME plan: per row max|dP| / max|W|^2 <= 32 eps of the precision, NaN where W is
NaN.  Then the strides (padding columns and rows not asked for keep a sentinel), the other entry points, the real-input
reductions, the Python shim against `cwt` and against the reference's fixtures, and the absence of state between calls.
"""
import numpy as np
import pytest

import pycwt_amd
from conftest import load_golden
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_kernels_emulated import grid

EPS32 = {64: 32 * np.finfo(np.float64).eps, 32: 32 * np.finfo(np.float32).eps}     # 7.1e-15, 3.8e-6
SENTINEL = -7.0


def types(prec):
    return (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)


def power_bound(P, W, prec):
    """per-row max|P - |W|^2| / max|W|^2 <= 32 eps, NaN positions identical"""
    W = np.asarray(W).astype(np.complex128)
    ref = W.real ** 2 + W.imag ** 2
    P = np.asarray(P, dtype=np.float64)
    assert P.shape == ref.shape
    assert np.array_equal(np.isnan(P), np.isnan(ref))
    ok = ~np.isnan(ref)
    d = np.where(ok, np.abs(P - ref), 0.0).max(axis=-1)
    peak = np.where(ok, ref, 0.0).max(axis=-1)
    err = d / np.where(peak == 0, 1.0, peak)
    assert err.max() <= EPS32[prec], (err.max(), EPS32[prec])
    return err


def both_outputs(lib, N, x, kind, param, sj, prec, opts, with_signal=True, ldp_pad=0, extra_rows=0):
    """(W, P, split) of one plan: cwt_transform (or forward FFT + cwt_transform_rows) and the power sibling, P written into
    an (rows + extra_rows) x (n0 + ldp_pad) matrix prefilled with SENTINEL (returned whole)."""
    real, cplx = types(prec)
    es = np.dtype(real).itemsize
    n0, rows = x.size, len(sj)
    ldp = n0 + ldp_pad
    plan = _hip.Plan(N, prec, max_rows=rows, lib=lib, options=opts)
    xd, xh = _hip.DeviceBuffer(n0 * es, lib=lib), _hip.DeviceBuffer(2 * es * N, lib=lib)
    Wd = _hip.DeviceBuffer(2 * es * rows * n0, lib=lib)
    Pd = _hip.DeviceBuffer(es * (rows + extra_rows) * ldp, lib=lib)
    try:
        xd.upload(plan, x.astype(real))
        Pd.upload(plan, np.full((rows + extra_rows, ldp), SENTINEL, dtype=real))
        if with_signal:
            plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
            split = plan.last_split()
            plan.transform_power(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Pd.ptr, ldp, n0)
        else:
            plan.forward_fft(xd.ptr, n0, xh.ptr)
            plan.transform_rows(xh.ptr, kind, param, 1.0, sj, Wd.ptr, n0, n0)
            split = plan.last_split()
            plan.transform_rows_power(xh.ptr, kind, param, 1.0, sj, Pd.ptr, ldp, n0)
        assert plan.last_split() == split          # the same row table, the same forms
        W = Wd.download(plan, (rows, n0), cplx)
        P = Pd.download(plan, (rows + extra_rows, ldp), real)
    finally:
        for b in (xd, xh, Wd, Pd):
            b.free()
        plan.close()
    return W, P, split


# (name, N, n0, mother, param, rows, options, the form that must carry rows)
FORMS = [
    ("direct", 8, 8, orc.MORLET, 6, 4, {}, "small"),
    ("single_wg", 1 << 10, 1000, orc.MORLET, 6, 24, {}, "small"),
    ("narrow_two_pass", 1 << 15, (1 << 15) - 3, orc.MORLET, 6, 40, {"ols": 0, "poly": 0}, "two_pass"),
    ("narrow_generic", 1 << 12, 4000, orc.MORLET, 6, 24, {"lmax": 128, "wg_points": 2048, "narrow_max_k": 256, "ols": 0,
                                                          "poly": 0}, "narrow"),
    ("ols", 1 << 15, (1 << 15) - 77, orc.MORLET, 6, 48, {"ols_min_logn": 15, "poly": 0}, "ols"),
    ("aols_paul", 1 << 16, (1 << 16) - 77, orc.PAUL, 4, 96, {"ols_min_logn": 15, "poly": 0}, {64: "narrow", 32: "aols"}),
    ("aols_morlet", 1 << 15, (1 << 15) - 11, orc.MORLET, 6, 48, {"ols_min_logn": 15, "poly": 0}, "aols"),
    ("aols_dog", 1 << 15, 1 << 15, orc.DOG, 2, 48, {"ols_min_logn": 15, "poly": 0}, "aols"),
    ("aols_dog_odd", 1 << 15, (1 << 15) - 7, orc.DOG, 3, 48, {"ols_min_logn": 15, "poly": 0}, "aols"),
    ("poly", 1 << 16, (1 << 16) - 37, orc.MORLET, 6, 64, {"poly_min_logn": 14}, "poly"),
    ("poly_dog", 1 << 15, (1 << 15) - 100, orc.DOG, 2, 48, {"poly_min_logn": 14}, "poly"),
]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", FORMS, ids=[f[0] for f in FORMS])
def test_every_row_form_power_equals_abs2_of_the_same_plan(emu_library, prec, name, N, n0, kind, param, rows, opts, form):
    x = np.random.default_rng(7).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    W, P, split = both_outputs(emu_library, N, x, kind, param, sj, prec, opts)
    form = form[prec] if isinstance(form, dict) else form
    assert split[form] > 0, split
    power_bound(P, W, prec)


@pytest.mark.parametrize("prec", [64, 32])
def test_spectrum_entry_point_power(emu_library, prec):
    """cwt_transform_rows_power (no signal: no overlap-save rows) against cwt_transform_rows of the same plan"""
    n0 = (1 << 15) - 11
    x = np.random.default_rng(3).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(orc.MORLET, 6), 40)
    W, P, split = both_outputs(emu_library, 1 << 15, x, orc.MORLET, 6, sj, prec, {"poly_min_logn": 14}, with_signal=False)
    assert split["ols"] == 0
    power_bound(P, W, prec)


@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", [FORMS[1], FORMS[4], FORMS[6], FORMS[9]],
                         ids=["single_wg", "ols", "aols", "poly"])
def test_strides_leave_padding_and_other_rows_alone(emu_library, name, N, n0, kind, param, rows, opts, form):
    x = np.random.default_rng(9).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    W, P, _ = both_outputs(emu_library, N, x, kind, param, sj, 64, opts, ldp_pad=13, extra_rows=2)
    assert np.all(P[:len(sj), n0:] == SENTINEL)
    assert np.all(P[len(sj):] == SENTINEL)
    power_bound(P[:len(sj), :n0], W, 64)


@pytest.mark.parametrize("prec,kind,param", [(64, orc.MORLET, 6), (32, orc.DOG, 2), (64, orc.PAUL, 4)])
def test_batch_power(emu_library, prec, kind, param):
    real, cplx = types(prec)
    es = np.dtype(real).itemsize
    N, nb = 1 << 15, 3
    n0 = N - 200
    X = np.random.default_rng(12).standard_normal((nb, n0))
    sj = grid(n0, 1.0, orc.Mother(kind, param), 24)
    rows = len(sj)
    plan = _hip.Plan(N, prec, max_rows=nb * rows, lib=emu_library, options={"ols_min_logn": 15, "poly_min_logn": 14})
    xd, xh = _hip.DeviceBuffer(nb * n0 * es, lib=emu_library), _hip.DeviceBuffer(nb * N * 2 * es, lib=emu_library)
    Wd, Pd = _hip.DeviceBuffer(nb * rows * n0 * 2 * es, lib=emu_library), _hip.DeviceBuffer(nb * rows * n0 * es, lib=emu_library)
    try:
        xd.upload(plan, X.astype(real))
        plan.transform_batch(xd.ptr, nb, n0, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        plan.transform_batch_power(xd.ptr, nb, n0, n0, kind, param, 1.0, sj, xh.ptr, Pd.ptr, n0, n0)
        W = Wd.download(plan, (nb * rows, n0), cplx)
        P = Pd.download(plan, (nb * rows, n0), real)
    finally:
        for b in (xd, xh, Wd, Pd):
            b.free()
        plan.close()
    power_bound(P, W, prec)


def test_rows_power_of_a_non_finite_signal_is_all_nan(emu_library):
    n0 = 4000
    x = np.random.default_rng(1).standard_normal(n0)
    x[1234] = np.nan
    sj = grid(n0, 1.0, orc.Mother(orc.MORLET, 6), 20)
    W, P, _ = both_outputs(emu_library, 1 << 12, x, orc.MORLET, 6, sj, 64, {}, with_signal=False)
    assert np.isnan(P).all() and np.isnan(W).all()


@pytest.mark.parametrize("n0,rows,N", [(504, 85, 512), (1 << 16, 24, 1 << 16)], ids=["canonical", "staged"])
def test_execute_host_power_paths_agree_with_the_device_path(emu_library, n0, rows, N):
    """The direct-to-page-locked small call (504 x 85) and the staged / copied path (2^16 samples) of cwt_execute_host_power
    give the bits of cwt_transform_power on the device, and the spectrum of cwt_execute_host."""
    x = np.random.default_rng(4).standard_normal(n0)
    sj = grid(n0, 0.25, orc.Mother(orc.MORLET, 6), rows)
    plan = _hip.Plan(N, 64, max_rows=rows, lib=emu_library)
    try:
        P_host, xh_p = plan.execute_host_power(x, orc.MORLET, 6, 0.25, sj)
        P_host = np.array(P_host)
        W_host, xh_w = plan.execute_host(x, orc.MORLET, 6, 0.25, sj)
        W_host = np.array(W_host)
        xd, xh = _hip.DeviceBuffer(n0 * 8, lib=emu_library), _hip.DeviceBuffer(N * 16, lib=emu_library)
        Pd = _hip.DeviceBuffer(rows * n0 * 8, lib=emu_library)
        xd.upload(plan, x)
        plan.transform_power(xd.ptr, n0, orc.MORLET, 6, 0.25, sj, xh.ptr, Pd.ptr, n0, n0)
        P_dev = Pd.download(plan, (rows, n0), np.float64)
        for b in (xd, xh, Pd):
            b.free()
    finally:
        plan.close()
    assert P_host.shape == (rows, n0) and P_host.dtype == np.float64
    assert np.array_equal(P_host, P_dev)
    assert np.array_equal(xh_p, xh_w)
    power_bound(P_host, W_host, 64)


@pytest.mark.parametrize("prec", [64, 32])
def test_real_input_reductions_match_numpy(emu_library, prec):
    real, _ = types(prec)
    es = np.dtype(real).itemsize
    rows, n0, ldp = 37, 3001, 3010
    P = np.abs(np.random.default_rng(2).standard_normal((rows, ldp))).astype(real)
    w = np.random.default_rng(5).uniform(0, 1, rows)
    plan = _hip.Plan(16, prec, max_rows=rows, lib=emu_library)
    Pd = _hip.DeviceBuffer(rows * ldp * es, lib=emu_library)
    g, s = _hip.DeviceBuffer(rows * es, lib=emu_library), _hip.DeviceBuffer(n0 * es, lib=emu_library)
    try:
        Pd.upload(plan, P)
        plan.time_mean_real(Pd.ptr, ldp, n0, rows, g.ptr)
        plan.reduce_scales(Pd.ptr, ldp, n0, w, 2, 0.7, s.ptr)
        gm = g.download(plan, (rows,), real)
        sa = s.download(plan, (n0,), real)
    finally:
        for b in (Pd, g, s):
            b.free()
        plan.close()
    P64 = P.astype(np.float64)[:, :n0]
    tol = 1e-13 if prec == 64 else 2e-6
    np.testing.assert_allclose(gm, P64.mean(axis=1), rtol=tol)
    np.testing.assert_allclose(sa, 0.7 * (w[:, None] * P64).sum(axis=0), rtol=tol)


def test_reduce_scales_rejects_unknown_power_values(emu_library):
    plan = _hip.Plan(16, 64, max_rows=4, lib=emu_library)
    try:
        with pytest.raises(Exception):
            plan.reduce_scales(1 << 20, 8, 8, np.ones(4), 3, 1.0, 1 << 20)
    finally:
        plan.close()


# ---- the Python shim ------------------------------------------------------------------------------------------------------
def check_against_cwt(a, b, prec=64):
    power_bound(a[0], b[0], prec)
    assert a[0].dtype == np.float64
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v, equal_nan=True)
        assert np.asarray(u).dtype == np.asarray(v).dtype


@pytest.mark.parametrize("mother", [pycwt_amd.Morlet(6), pycwt_amd.Paul(4), pycwt_amd.DOG(2), pycwt_amd.MexicanHat()],
                         ids=["morlet", "paul", "dog", "mexican_hat"])
def test_cwt_power_equals_abs2_of_cwt(emulated, mother):
    x = np.random.default_rng(8).standard_normal(3000)
    check_against_cwt(pycwt_amd.cwt_power(x, 0.5, 1 / 8, -1, -1, mother), pycwt_amd.cwt(x, 0.5, 1 / 8, -1, -1, mother))


def test_cwt_power_long_series_with_overlap_save_and_polynomial_rows(emulated):
    x = np.random.default_rng(18).standard_normal((1 << 18) - 11)
    a = pycwt_amd.cwt_power(x, 1.0, 0.5, -1, -1, "morlet")
    b = pycwt_amd.cwt(x, 1.0, 0.5, -1, -1, "morlet")
    assert next(iter(pycwt_amd.wavelet._plans.values())).last_split()["ols"] > 0
    check_against_cwt(a, b)


def test_cwt_power_float32_input_and_precision(emulated):
    x = np.random.default_rng(6).standard_normal(2000).astype(np.float32)
    check_against_cwt(pycwt_amd.cwt_power(x, 1.0, 1 / 4), pycwt_amd.cwt(x, 1.0, 1 / 4))
    check_against_cwt(pycwt_amd.cwt_power(x, 1.0, 1 / 4, precision=32), pycwt_amd.cwt(x, 1.0, 1 / 4, precision=32), 32)


def test_cwt_power_complex_input_is_the_power_of_the_combined_transform(emulated):
    rng = np.random.default_rng(10)
    z = rng.standard_normal(1500) + 1j * rng.standard_normal(1500)
    a = pycwt_amd.cwt_power(z, 1.0, 1 / 4)
    b = pycwt_amd.cwt(z, 1.0, 1 / 4)
    check_against_cwt(a, b)
    ar = pycwt_amd.cwt_power(z.real, 1.0, 1 / 4)[0] + pycwt_amd.cwt_power(z.imag, 1.0, 1 / 4)[0]
    assert not np.allclose(a[0], ar)                      # not the sum of the two powers


class DuckMorlet:
    """A mother wavelet without device_id(): the reference's duck-typed protocol"""
    def __init__(self):
        self.m = pycwt_amd.Morlet(6)

    def psi_ft(self, f):
        return self.m.psi_ft(f)

    def flambda(self):
        return self.m.flambda()

    def coi(self):
        return self.m.coi()


def test_cwt_power_duck_typed_mother_and_unpadded(emulated):
    x = np.random.default_rng(11).standard_normal(1200)
    check_against_cwt(pycwt_amd.cwt_power(x, 1.0, 1 / 4, wavelet=DuckMorlet()), pycwt_amd.cwt(x, 1.0, 1 / 4, wavelet=DuckMorlet()))
    check_against_cwt(pycwt_amd.cwt_power(x, 1.0, 1 / 4, pad=False), pycwt_amd.cwt(x, 1.0, 1 / 4, pad=False))


def test_cwt_power_nan_sample_and_paul_nan_rows(emulated):
    x = np.random.default_rng(12).standard_normal(5000)
    x[17] = np.nan
    a = pycwt_amd.cwt_power(x, 1.0, 1 / 4, -1, -1, pycwt_amd.Paul(4))
    b = pycwt_amd.cwt(x, 1.0, 1 / 4, -1, -1, pycwt_amd.Paul(4))
    assert np.isnan(a[0]).all()
    check_against_cwt(a, b)
    y = np.random.default_rng(13).standard_normal(5000)
    check_against_cwt(pycwt_amd.cwt_power(y, 1.0, 1 / 4, -1, -1, pycwt_amd.Paul(4)),
                      pycwt_amd.cwt(y, 1.0, 1 / 4, -1, -1, pycwt_amd.Paul(4)))


def test_cwt_power_automatic_tolerance(emulated):
    x = np.random.default_rng(14).standard_normal(20000)
    pycwt_amd.set_tolerance("auto")
    a = pycwt_amd.cwt_power(x, 1.0, 1 / 4)
    b = pycwt_amd.cwt(x, 1.0, 1 / 4)
    check_against_cwt(a, b)


def test_cwt_power_batch(emulated):
    X = np.random.default_rng(15).standard_normal((3, 3000))
    X[2, 100] = np.inf
    a = pycwt_amd.cwt_power_batch(X, 1.0, 1 / 4, -1, -1, "dog")
    b = pycwt_amd.cwt_batch(X, 1.0, 1 / 4, -1, -1, "dog")
    assert a[0].shape == b[0].shape and np.isnan(a[0][2]).all()
    power_bound(a[0], b[0], 64)
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v, equal_nan=True)
    finite = pycwt_amd.cwt_power_batch(X[:2], 1.0, 1 / 4, -1, -1, "dog", max_batch_bytes=1)      # one signal per slab
    assert np.array_equal(finite[0], a[0][:2]) or power_bound(finite[0], b[0][:2], 64) is not None


def test_device_power_handle(emulated):
    x = np.random.default_rng(16).standard_normal(4096)
    h = pycwt_amd.cwt_power_device(x, 1.0, 1 / 4)
    ref = pycwt_amd.cwt(x, 1.0, 1 / 4)
    try:
        P = h.power()
        power_bound(P, ref[0], 64)
        assert not hasattr(h, "W") and not hasattr(h, "icwt")
        np.testing.assert_allclose(h.global_power(), P.mean(axis=1), rtol=1e-13)
        sa = h.scale_average(2.0, 8.0, 1 / 4)
        w = np.where((ref[1] >= 2.0) & (ref[1] < 8.0), 1.0 / ref[1], 0.0)
        np.testing.assert_allclose(sa, 0.25 * 1.0 / h.mother.cdelta * (w[:, None] * P).sum(axis=0), rtol=1e-12, atol=1e-300)
        assert np.array_equal(h.fft, ref[4]) and h.device_ptr
        assert np.array_equal(h.sj, ref[1]) and np.array_equal(h.coi, ref[3])
    finally:
        h.close()


@pytest.mark.parametrize("name,cls", [("morlet", pycwt_amd.Morlet), ("paul", pycwt_amd.Paul), ("dog", pycwt_amd.DOG)])
def test_small_fixtures_against_the_reference(emulated, name, cls):
    g = load_golden("small_" + name)
    P = pycwt_amd.cwt_power(g["x"], float(g["dt"]), float(g["dj"]), -1, -1, cls())[0]
    ref = np.abs(g["W"]) ** 2
    assert P.shape == ref.shape
    peak = np.nanmax(ref, axis=1, keepdims=True)
    np.testing.assert_array_less(np.abs(P - ref) / peak, 1e-12)


@pytest.mark.parametrize("name,cls", [("morlet", pycwt_amd.Morlet), ("paul", pycwt_amd.Paul), ("dog", pycwt_amd.DOG)])
def test_mid_fixtures_against_the_reference(emulated, name, cls):
    g = load_golden("mid_" + name)
    x = np.random.default_rng(int(g["seed"])).standard_normal(int(g["N"]))
    m = cls()
    P, sj = pycwt_amd.cwt_power(x, float(g["dt"]), freqs=1 / (m.flambda() * g["sj"]), wavelet=m)[:2]
    np.testing.assert_allclose(sj, g["sj"], rtol=1e-15)
    ref = np.abs(g["W"]) ** 2
    peak = ref.max(axis=1, keepdims=True)
    np.testing.assert_array_less(np.abs(P - ref) / peak, 1e-12)


def test_no_state_leaks_into_the_complex_path(emulated):
    """cwt after cwt_power on the same cached plan gives the bits it gave before"""
    x = np.random.default_rng(17).standard_normal((1 << 16) - 5)
    before = pycwt_amd.cwt(x, 1.0, 1 / 2)
    pycwt_amd.cwt_power(x, 1.0, 1 / 2)
    after = pycwt_amd.cwt(x, 1.0, 1 / 2)
    assert len(pycwt_amd.wavelet._plans) == 1
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
