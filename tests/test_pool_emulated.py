"""The time-pooled scalogram -- cwt_transform_pool and the `pool=` keyword of cwt_power, cwt_power_device, cwt_power_batch and
cwt_power_torch -- on the CPU emulation of the HIP runtime (tests/emu).

Reference and bound (tests/pool_common.py): the same plan's cwt_transform_power output pooled on the host in long double, per row
max_m |Pbar - ref| / max_m ref <= 4 x the ratio measured over these cases on the emulation (profiles/pool_accuracy.txt:
4.564e-16 / 2.741e-07 measured, 1.826e-15 / 1.096e-06 asserted); independently the oracle pooled the same way, within 2 x the
round-off tolerance of tests/test_gpu_parity.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pool_common as pc
import pycwt_amd
from oracle import cwt_oracle as orc
from test_adjoint_emulated import BOUND as ADJOINT_BOUND, rel
from test_hop_emulated import launch_log, schedule, fresh_engines, LOCKSTEP, WAVE_SCHEDULES        # noqa: F401 (fixtures)
from test_kernels_emulated import grid

PRECS = [64, 32]
EINVAL = -1


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", pc.FORMS, ids=[f[0] for f in pc.FORMS])
def test_every_row_form_pooled_equals_the_pooled_power_of_the_same_plan(emu_library, form, prec):
    """FORMS of test_power_emulated (ragged n0: the last window is short) x pool in {2, 64, 4096} (<= nfft) and pool = nfft on two
    of them: the expected form carries rows, the split is the power call's, ldp padding and extra rows keep the sentinel."""
    errs = pc.check_form(emu_library, form, prec, pc.BOUND[prec])
    assert sorted(errs) == sorted(pc.form_pools(form))


def test_the_pools_cover_a_window_inside_equal_to_and_over_many_intervals():
    """at N = 2^15 ... 2^16 the polynomial intervals are R = 64 ... 256 samples: 2 < R, 64 = the shortest R, 4096 = many"""
    assert min(pc.FORM_POOLS) < 64 and 64 in pc.FORM_POOLS and max(pc.FORM_POOLS) >= 16 * 256
    assert sum(1 for f in pc.FORMS if f[0] in pc.NFFT_POOL_FORMS) == 2


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("tolerance", [pc.POLY_TOLERANCE, 0.0], ids=["tol1e-9", "round-off"])
def test_polynomial_rows_by_interval_count_and_degree(emu_library, tolerance, prec):
    """rows IDX of poly_xcd_common at N = 2^16, pool in {16, 128, 1024}: at 1e-9 its (K', D) pairs WANT, at round-off the highest
    degrees"""
    errs, have = pc.check_poly_rows(emu_library, prec, tolerance, pc.BOUND[prec], want=pc.WANT if tolerance else None)
    assert sorted(errs) == sorted(pc.POLY_POOLS)
    if not tolerance and prec == 64:
        assert max(d for _, d in have) > max(d for _, d in pc.WANT), have


@pytest.mark.parametrize("prec", PRECS)
def test_signal_shorter_than_half_the_next_check(emu_library, prec):
    """n0 = 2^15 + 1 on N = 2^16, pool 4096: exactly 9 windows, the last of one column"""
    pc.check_short_signal(emu_library, prec, pc.BOUND[prec])


@pytest.mark.parametrize("prec", PRECS)
def test_against_the_oracle(emu_library, prec):
    """the independent check: the oracle's |W|^2 pooled the same way, per row relative to the row's peak power"""
    N, n0, sj, x, Pref = pc.oracle_case(prec)
    peak = Pref.max(axis=1)
    with pc.Device(emu_library, N, prec, max_rows=len(sj), options={"poly_min_logn": 14, "ols_min_logn": 15}) as dev:
        for pool in (2, 64, 4096):
            B = pc.run_pool(dev, x, pc.MORLET, pc.F0, sj, pool)
            err = (np.abs(B.astype(np.longdouble) - pc.window_means(Pref, pool)).max(axis=1) / peak).max()
            print("against the oracle: pool", pool, "precision", prec, float(err), "bound", pc.ORACLE_BOUND[prec])
            assert err <= pc.ORACLE_BOUND[prec], (pool, float(err))
        assert dev.plan.last_split()["poly"] > 0 and dev.plan.last_split()["ols"] > 0


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_bits_do_not_depend_on_the_batch_the_run_or_the_calls_around(emu_library, prec):
    """A signal alone and as member 1 of a batch of 3 (x_ld > n0, spectra asked for and not): the same bits; two runs: the same
    bits; a pooled call between two transform calls leaves their outputs bit-identical and last_split() unchanged."""
    N, n0, pool = 1 << 15, (1 << 15) - 77, 64
    sj = grid(n0, 1.0, orc.Mother(pc.MORLET, pc.F0), 40)
    rows = len(sj)
    X = np.random.default_rng(31).standard_normal((3, n0))
    with pc.Device(emu_library, N, prec, max_rows=3 * rows, options={"poly_min_logn": 14, "ols_min_logn": 15}) as dev:
        xd, Wd = dev.up(X[1].astype(dev.real)), dev.up(np.zeros((rows, n0), dtype=dev.cplx))
        dev.plan.transform(xd.ptr, n0, pc.MORLET, pc.F0, 1.0, sj, None, Wd.ptr, n0, n0)
        W0, split = Wd.download(dev.plan, (rows, n0), dev.cplx), dev.plan.last_split()
        assert split["poly"] > 0 and split["ols"] > 0
        one = pc.run_pool(dev, X[1], pc.MORLET, pc.F0, sj, pool)
        assert dev.plan.last_split() == split
        dev.plan.transform(xd.ptr, n0, pc.MORLET, pc.F0, 1.0, sj, None, Wd.ptr, n0, n0)
        assert np.array_equal(Wd.download(dev.plan, (rows, n0), dev.cplx).view(np.uint8), W0.view(np.uint8))
        assert dev.plan.last_split() == split
        again = pc.run_pool(dev, X[1], pc.MORLET, pc.F0, sj, pool)
        assert np.array_equal(one.view(np.uint8), again.view(np.uint8))
        batch = pc.run_pool(dev, X, pc.MORLET, pc.F0, sj, pool)
        assert np.array_equal(batch[rows:2 * rows].view(np.uint8), one.view(np.uint8))
        xh = dev.up(np.zeros((3, N), dtype=dev.cplx))
        Xp = np.full((3, n0 + 5), np.nan)
        Xp[:, :n0] = X
        nc = -(-n0 // pool)
        out, xp = dev.up(np.full((3 * rows, nc), pc.SENTINEL, dtype=dev.real)), dev.up(Xp.astype(dev.real))
        dev.plan.transform_pool(xp.ptr, 3, n0 + 5, n0, pc.MORLET, pc.F0, 1.0, sj, pool, xh.ptr, out.ptr, nc)
        assert np.array_equal(out.download(dev.plan, (3 * rows, nc), dev.real).view(np.uint8), batch.view(np.uint8))
        spectra = xh.download(dev.plan, (3, N), dev.cplx)
        assert np.abs(spectra).min(axis=1).max() > 0 and not np.isnan(spectra).any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_write_nothing(emu_library):
    lib, dll = emu_library, emu_library.dll
    N, n0, pool = 1 << 12, 4000, 16
    nc = -(-n0 // pool)
    sj = np.ascontiguousarray(grid(n0, 1.0, orc.Mother(pc.MORLET, pc.F0), 12))
    rows = len(sj)
    sp = sj.ctypes.data_as(C.POINTER(C.c_double))
    P = C.c_void_p
    with pc.Device(lib, N, 64, max_rows=rows) as dev:
        xd, out = dev.up(np.zeros(n0)), dev.up(np.full((rows, nc), pc.SENTINEL))

        def call(x=xd.ptr, s=sp, o=out.ptr, pool_=pool, ld=nc, ncp=nc, nbatch=1):
            return dll.cwt_transform_pool(dev.plan.h, P(x), nbatch, n0, n0, 0, 6.0, 1.0, s, rows, pool_, None, P(o), ld, ncp)
        dev.plan.sync()
        dll.hipemu_clear_launched()
        refused = [("pool not a power of two", call(pool_=12, ncp=-(-n0 // 12), ld=400)), ("pool = 1", call(pool_=1, ncp=n0, ld=n0)),
                   ("pool = 0", call(pool_=0)), ("pool < 0", call(pool_=-4)), ("pool > nfft", call(pool_=2 * N, ncp=1)),
                   ("ncols_p too small", call(ncp=nc - 1)), ("ncols_p too large", call(ncp=nc + 1, ld=nc + 1)), ("ldp < ncols_p", call(ld=nc - 1)),
                   ("x NULL", call(x=None)), ("P NULL", call(o=None)), ("scales NULL", call(s=None)), ("rows > max_rows", call(nbatch=2))]
        for name, rc in refused:
            assert rc == EINVAL and lib.cwt_last_error(), name
        assert launch_log(lib) == set()
        assert np.all(out.download(dev.plan, (rows, nc), np.float64) == pc.SENTINEL)
        assert call() == 0 and any("pool_rows" in s for s in launch_log(lib))            # ... and the good call goes through
        assert call(pool_=N, ncp=1, ld=1) == 0                                          # pool = nfft is the largest allowed


# ---- the Python functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", ["morlet", "paul", "dog"])
def test_cwt_power_with_pool(emulated, wavelet):
    n0, pool = 4019, 16
    x = np.random.default_rng(6).standard_normal(n0)
    P, sj, freqs, coi, fft5, fftfreqs = pycwt_amd.cwt_power(x, 0.25, 1 / 2, wavelet=wavelet)
    Pp, sjp, freqsp, coip, fft5p, fftfreqsp = pycwt_amd.cwt_power(x, 0.25, 1 / 2, wavelet=wavelet, pool=pool)
    assert Pp.shape == (len(sj), -(-n0 // pool)) and Pp.dtype == np.float64
    for a, b in ((sj, sjp), (freqs, freqsp), (fftfreqs, fftfreqsp)):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(fft5p, fft5, rtol=0, atol=1e-13 * np.abs(fft5).max())
    assert pc.row_ratio(Pp, pc.window_means(P, pool)).max() <= pc.BOUND[64]
    # the coi rule: the minimum over the window, the last (short) window over its own columns
    want = np.array([coi[m * pool:(m + 1) * pool].min() for m in range(-(-n0 // pool))])
    assert np.array_equal(coip, want) and coip[-1] == coi[-1] and coip[0] == coi[0]


def test_python_refusals_nan_and_float32(emulated):
    x = np.random.default_rng(7).standard_normal(3000)
    with pytest.raises(ValueError, match="pool and hop"):
        pycwt_amd.cwt_power(x, 1.0, pool=4, hop=4)
    with pytest.raises(ValueError, match="power of two"):
        pycwt_amd.cwt_power(x, 1.0, pool=3)
    with pytest.raises(ValueError, match="power of two"):
        pycwt_amd.cwt_power(x, 1.0, pool=1)
    with pytest.raises(ValueError, match="padded length"):
        pycwt_amd.cwt_power(x, 1.0, pool=8192)
    with pytest.raises(ValueError, match="pad"):
        pycwt_amd.cwt_power(x, 1.0, pool=4, pad=False)
    with pytest.raises(ValueError, match="real signals"):
        pycwt_amd.cwt_power(x + 1j, 1.0, pool=4)
    with pytest.raises(ValueError, match="pool and hop"):
        pycwt_amd.cwt_power_batch(x[None], 1.0, pool=4, hop=4)
    y = x.copy()
    y[17] = np.nan
    out = pycwt_amd.cwt_power(y, 1.0, 1 / 4, pool=8)
    assert out[0].shape[1] == 375 and np.isnan(out[0]).all() and np.isnan(out[4]).all()
    a = pycwt_amd.cwt_power(x.astype(np.float32), 1.0, 1 / 4, precision=32)
    b = pycwt_amd.cwt_power(x.astype(np.float32), 1.0, 1 / 4, precision=32, pool=8)
    assert b[0].dtype == np.float64 and pc.row_ratio(b[0], pc.window_means(a[0].astype(np.float32), 8)).max() <= pc.BOUND[32]


@pytest.mark.parametrize("wavelet", ["morlet", "dog"])
def test_device_result_and_batch_with_pool(emulated, wavelet):
    n0, pool = 9001, 32                                                  # (nfft = 2^14 > 4096: the batch runs at the plan's tolerance)
    rng = np.random.default_rng(16)
    X = rng.standard_normal((3, n0))
    X[2, 100] = np.inf
    full = pycwt_amd.cwt_power(X[0], 0.25, 1 / 2, wavelet=wavelet)
    single = pycwt_amd.cwt_power(X[0], 0.25, 1 / 2, wavelet=wavelet, pool=pool)
    dp = pycwt_amd.cwt_power_device(X[0], 0.25, 1 / 2, wavelet=wavelet, pool=pool)
    try:
        assert dp.shape == single[0].shape and np.array_equal(dp.coi, single[3]) and np.array_equal(dp.sj, single[1])
        assert np.array_equal(dp.power(), single[0])                    # the same export on the same plan
        np.testing.assert_allclose(dp.global_power(), single[0].mean(axis=1), rtol=1e-12)
    finally:
        dp.close()
    Pb, sjb, _, coib, fftb, _ = pycwt_amd.cwt_power_batch(X, 0.25, 1 / 2, wavelet=wavelet, pool=pool)
    assert Pb.shape == (3,) + single[0].shape and np.array_equal(coib, single[3]) and np.array_equal(sjb, single[1])
    assert pc.row_ratio(Pb[0], pc.window_means(full[0], pool)).max() <= pc.BOUND[64]
    assert pc.row_ratio(Pb[1], pc.window_means(pycwt_amd.cwt_power(X[1], 0.25, 1 / 2, wavelet=wavelet)[0], pool)).max() <= pc.BOUND[64]
    assert np.isnan(Pb[2]).all() and np.isnan(fftb[2]).all() and not np.isnan(Pb[:2]).any()
    slabs = pycwt_amd.cwt_power_batch(X[:2], 0.25, 1 / 2, wavelet=wavelet, pool=pool, max_batch_bytes=1)[0]
    assert np.array_equal(slabs, pycwt_amd.cwt_power_batch(X[:2], 0.25, 1 / 2, wavelet=wavelet, pool=pool)[0])


# ---- torch ------------------------------------------------------------------------------------------------------------------------
def test_gradcheck_with_pool(fresh_engines):
    torch = pytest.importorskip("torch")
    x = torch.randn((2, 500), dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 2.0, wavelet="dog", pool=4)[0], (x,), atol=1e-8)


def window_mean_torch(torch, P, pool):
    n0 = P.shape[-1]
    nc = -(-n0 // pool)
    padded = torch.nn.functional.pad(P, (0, nc * pool - n0))
    count = torch.full((nc,), float(pool), dtype=P.dtype)
    count[-1] = n0 - (nc - 1) * pool
    return padded.reshape(P.shape[:-1] + (nc, pool)).sum(dim=-1) / count


@pytest.mark.parametrize("prec", PRECS)
def test_torch_values_and_gradient_against_the_explicit_window_mean(fresh_engines, prec):
    """N = 2^15, ragged n0, pool 64: values against the window means of cwt_power_torch (BOUND), x alone saved, and x.grad against
    the gradient of the same loss through cwt_power_torch and an explicit window mean in torch -- the two routes hand the adjoint
    the same G up to rounding: BOUND of test_adjoint_emulated, as in test_power_torch_emulated."""
    torch = pytest.importorskip("torch")
    real_t = torch.float64 if prec == 64 else torch.float32
    n0, pool = (1 << 15) - 77, 64
    rng = np.random.default_rng(41)
    x0 = torch.as_tensor(rng.standard_normal(n0), dtype=real_t)
    xa = x0.clone().requires_grad_(True)
    P, sj, freqs, coi = pycwt_amd.cwt_power_torch(xa, 1.0, 1 / 4, wavelet="morlet")
    xb = x0.clone().requires_grad_(True)
    Pp, sjp, freqsp, coip = pycwt_amd.cwt_power_torch(xb, 1.0, 1 / 4, wavelet="morlet", pool=pool)
    nc = -(-n0 // pool)
    assert Pp.shape == (len(sj), nc) and Pp.dtype == real_t and np.array_equal(sj, sjp) and np.array_equal(freqs, freqsp)
    assert coip.shape == (nc,) and coip[3] == coi[3 * pool:4 * pool].min()
    assert pc.row_ratio(Pp.detach().numpy(), pc.window_means(P.detach().numpy(), pool)).max() <= pc.BOUND[prec]
    saved = Pp.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].shape == xb.shape
    gP = torch.as_tensor(rng.standard_normal((len(sj), nc)), dtype=real_t)
    (window_mean_torch(torch, P, pool) * gP).sum().backward()
    (Pp * gP).sum().backward()
    err = rel(xb.grad.numpy().astype(np.float64), xa.grad.numpy().astype(np.float64))
    print("pooled gradient against the explicit window mean, precision", prec, err)
    assert xb.grad.dtype == real_t and err <= ADJOINT_BOUND[prec], err
    with pytest.raises(ValueError, match="pool and hop"):
        pycwt_amd.cwt_power_torch(x0, 1.0, pool=4, hop=4)
    assert len(fresh_engines._engines) == 1


def test_torch_gradients_with_respect_to_scales_and_f0(fresh_engines):
    """pool= with scales= and f0=: the three gradients against the route through cwt_power_torch and the explicit window mean"""
    torch = pytest.importorskip("torch")
    n0, pool = 4019, 16
    rng = np.random.default_rng(43)
    x0 = torch.as_tensor(rng.standard_normal((2, n0)))
    t0 = torch.as_tensor(2.0 * 2 ** (np.arange(10) * 0.9))
    grads = []
    for pooled in (False, True):
        x, t = x0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
        f0 = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
        if pooled:
            out = pycwt_amd.cwt_power_torch(x, 1.0, wavelet="morlet", scales=t, f0=f0, pool=pool)[0]
        else:
            out = window_mean_torch(torch, pycwt_amd.cwt_power_torch(x, 1.0, wavelet="morlet", scales=t, f0=f0)[0], pool)
        if not grads:
            gP = torch.as_tensor(rng.standard_normal(tuple(out.shape)))
        (out * gP).sum().backward()
        grads.append((x.grad.numpy(), t.grad.numpy(), np.atleast_1d(f0.grad.numpy())))
    for a, b in zip(*grads):
        assert rel(b, a) <= ADJOINT_BOUND[64], rel(b, a)


def test_state_does_not_leak(emulated, monkeypatch):
    """cwt, cwt_power and cwt_power(hop=) give the same bits before and after pooled calls on the same plan (one cached table)"""
    n0 = (1 << 16) - 5
    xn = np.random.default_rng(35).standard_normal(n0)

    def all_three():
        return (pycwt_amd.cwt(xn, 1.0, 1 / 2)[0], pycwt_amd.cwt_power(xn, 1.0, 1 / 2)[0], pycwt_amd.cwt_power(xn, 1.0, 1 / 2, hop=16)[0])
    before = all_three()
    a = pycwt_amd.cwt_power(xn, 1.0, 1 / 2, pool=16)[0]
    after = all_three()
    assert np.array_equal(a, pycwt_amd.cwt_power(xn, 1.0, 1 / 2, pool=16)[0])
    assert len(pycwt_amd.wavelet._plans) == 1
    for u, v in zip(before, after):
        assert np.array_equal(u, v)


# ---- wavefront schedules (tests/emu/hipemu.cpp) -------------------------------------------------------------------------------------
POOL_KERNELS = {"pool_poly_rows", "pool_rows"}


def schedule_case(lib, pool, prec):
    """polynomial and other rows of one geometry, a batch of 2: every pool kernel, as bytes"""
    N = 1 << 14
    n0 = N - 77
    sj = grid(n0, 1.0, orc.Mother(pc.MORLET, pc.F0), 16)
    X = np.random.default_rng(9).standard_normal((2, n0))
    with pc.Device(lib, N, prec, max_rows=2 * len(sj), options={"poly_min_logn": 14}) as dev:
        B = pc.run_pool(dev, X, pc.MORLET, pc.F0, sj, pool)
        assert dev.plan.last_split()["poly"] > 0
    return B.view(np.uint8).copy()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("pool", [2, 8, 16, 256, 1024, 4096, 1 << 14])
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, pool, prec):
    """Forward, reverse and seeded wavefront orders give the bits of the lockstep order: whole windows inside a thread (pool 2,
    8), the tree over 1 ... 256 lanes, and a workgroup per window (pool > 4096 in pool_poly_rows, > 1024 in pool_rows).
    test_emu_schedules.py's coverage gate lists the kernels named k_*; the pool kernels are gated here: each of them is launched
    under every schedule."""
    schedule(LOCKSTEP)
    base = schedule_case(emu_library, pool, prec)
    for label, k, s in WAVE_SCHEDULES:
        schedule(k, s)
        emu_library.dll.hipemu_clear_launched()
        got = schedule_case(emu_library, pool, prec)
        log = launch_log(emu_library)
        assert all(any(name in s for s in log) for name in POOL_KERNELS), (label, log)
        assert np.array_equal(base, got), label


def test_every_pool_kernel_is_known_to_the_schedule_test():
    """the kernels of cwt_kernels_pool.hpp are exactly those the schedule test launches"""
    from conftest import ROOT
    text = open(os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_pool.hpp")).read()
    assert set(re.findall(r"__global__[^{;]*?\b(pool_\w+)\s*\(", text)) == POOL_KERNELS
