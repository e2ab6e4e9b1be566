"""The decimated transform -- cwt_transform_hop, cwt_transform_rows_hop, cwt_adjoint_rows_hop and the `hop=` keyword of the
Python functions -- on the CPU emulation of the HIP runtime (tests/emu).

Reference: the oracle's W (oracle/cwt_oracle.py, float64) with columns ::hop taken; per row, relative to the row's own peak in
the UNDECIMATED oracle row.  The bound is measured, not chosen (profiles/hop_accuracy.txt, tests/perf/hop_accuracy.py): on
the same inputs the existing cwt_transform at round-off has per-row errors of at most 4.038e-15 (fp64) / 8.556e-06 (fp32)
against the same oracle; a hop row may have 4 x that, 1.615e-14 / 3.423e-05 (the fold adds a sum of up to hop terms in working
precision before the transform).  The hop rows measured 4.162e-15 / 8.757e-06.  The gradient through cwt_torch(hop=h) against
the float64 NumPy adjoint: 4 x the 8.665e-16 / 4.026e-07 (relative L2) of the existing cwt_torch + slice; measured 7.4e-16 /
3.5e-07.  Cases, grids and references: tests/hop_common.py.
"""
import ctypes as C

import numpy as np
import pytest

import hop_common as hc
import pycwt_amd
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND as ADJOINT_BOUND, FORMS_OPTS, random_g, rel
from test_power_emulated import EPS32

PRECS = [64, 32]
CASE_IDS = [hc.case_id(c) for c in hc.CASES]
EINVAL = -1


def launch_log(lib):
    dll = lib.dll
    dll.hipemu_launched.restype = C.c_size_t
    dll.hipemu_launched.argtypes = [C.c_char_p, C.c_size_t]
    need = dll.hipemu_launched(None, 0)
    buf = C.create_string_buffer(need)
    dll.hipemu_launched(buf, need)
    return set(buf.value.decode().split("\n")) - {""}


def draw_q(seed, shape, real):
    """seeded normal weights, both signs, about 2 % exact zeros"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal(shape)
    Q[rng.random(shape) < 0.02] = 0.0
    return Q.astype(real)


# ---- values ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", hc.CASES, ids=CASE_IDS)
def test_hop_rows_against_the_oracle_power_and_weighted(emu_library, case, prec):
    """W_h per row within HOP_BOUND of oracle[:, ::hop]; the fold kernel and the fused fold give the same bits; the power is
    re^2 + im^2 of that W_h to 4 eps of the value; the weighted output is (alpha Q) W_h within 32 eps of the row peak, for
    alpha = 2 and -0.75 and a Q with exact zeros and both signs."""
    logn, hop, n0, kind, param = case
    sj, ref, peak = hc.reference(logn, n0, kind, param, prec)
    x = hc.signal(n0, prec)
    eps = float(np.finfo(hc.types(prec)[0]).eps)
    with hc.Device(emu_library, 1 << logn, prec) as dev:
        W = hc.run_hop(dev, x, kind, param, sj, hop)
        err = hc.row_error(W, ref[:, ::hop], peak)
        print("hop rows against the oracle:", hc.case_id(case), prec, err, "bound", hc.HOP_BOUND[prec])
        assert W.shape == (len(sj), -(-n0 // hop)) and err <= hc.HOP_BOUND[prec], (err, hc.HOP_BOUND[prec])
        P = hc.run_hop(dev, x, kind, param, sj, hop, output=1)
        Wd = W.astype(np.complex128)
        want = Wd.real ** 2 + Wd.imag ** 2
        assert P.dtype == dev.real and np.all(np.abs(P.astype(np.float64) - want) <= 4 * eps * want)
        Q = draw_q(11, W.shape, dev.real)
        for alpha in (2.0, -0.75):
            G = hc.run_hop(dev, x, kind, param, sj, hop, output=2, Q=Q, alpha=alpha).astype(np.complex128)
            want = alpha * Q.astype(np.float64) * Wd
            for got, w in ((G.real, want.real), (G.imag, want.imag)):
                e = np.abs(got - w).max(axis=1) / np.where(np.abs(w).max(axis=1) == 0, 1.0, np.abs(w).max(axis=1))
                assert e.max() <= EPS32[prec], (alpha, e.max())
        dev.plan.set_option("hop_fuse_terms", 0)                      # every row through the fold kernel and scratch
        W0 = hc.run_hop(dev, x, kind, param, sj, hop)
        dev.plan.set_option("hop_fuse_terms", 65536)                  # ... and none
        W1 = hc.run_hop(dev, x, kind, param, sj, hop)
    assert np.array_equal(W0.view(np.uint8), W.view(np.uint8)) and np.array_equal(W1.view(np.uint8), W.view(np.uint8))


def test_the_grid_reaches_both_ends_of_the_fold(emu_library):
    """What the cases are chosen for: rows with about N / 2 bins (hop aliases per folded bin), rows narrower than one alias
    (nband < M), and for DOG a negative k_lo that reaches the Nyquist bin -N / 2."""
    for logn, hop in hc.SHAPES:
        N, M = 1 << logn, (1 << logn) // hop
        for kind, param in hc.MOTHERS:
            sj = hc.scales(N, kind, param)
            bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, orc.Mother(kind, param), True)
            live = np.abs(bank) > 1e-16 * np.abs(bank).max(axis=1, keepdims=True)
            nband = live.sum(axis=1)
            assert nband.max() >= 0.99 * (N // 2 if kind != orc.DOG else N), (kind, nband.max())
            if kind != orc.PAUL:                  # (Paul's large scales are the rows the reference turns into NaN: dropped)
                assert nband.min() < M, (kind, nband.min(), M)
            if kind == orc.DOG:
                assert live[0, N // 2] and live[0, N // 2 + 1:].any()       # the Nyquist bin and negative bins of the first row


@pytest.mark.parametrize("prec", PRECS)
def test_single_tone_closed_form(emu_library, prec):
    """x = cos(2 pi k0 n / N), n0 = N: W[j, m h] = (F_j[k0] e^{i t} + F_j[N - k0] e^{-i t}) / 2, t = 2 pi k0 m h / N, with the
    phase in long double; k0 = the peak of a row in the middle of the grid, compared on the rows whose filter at k0 is at least
    half its peak (in a row that sees the tone through its filter's tail, the rounding of the samples is no longer small
    against the row).  HOP_BOUND relative to the row's peak."""
    N, hop = 1 << 12, 16
    for kind, param in hc.MOTHERS:
        sj = hc.scales(N, kind, param)
        real = hc.types(prec)[0]
        bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, orc.Mother(kind, param), True)
        k0 = 1 + int(np.argmax(np.abs(bank[len(sj) // 2, 1:N // 2])))
        two_pi = 8 * np.arctan(np.longdouble(1))               # (np.pi is a double: 1.2e-16 x 2 pi k0 of phase drift over the signal)
        x = np.cos(two_pi * ((k0 * np.arange(N)) % N).astype(np.longdouble) / N).astype(real)
        ref_full = orc.cwt_rows(x.astype(np.float64), 1.0, sj, orc.Mother(kind, param), N=N)
        t = two_pi * ((k0 * hop * np.arange(N // hop)) % N).astype(np.longdouble) / N
        closed = 0.5 * (bank[:, [k0]] * (np.cos(t) + 1j * np.sin(t)) + bank[:, [N - k0]] * (np.cos(t) - 1j * np.sin(t)))
        peak = np.abs(ref_full).max(axis=1)
        keep = np.abs(bank[:, k0]) >= 0.5 * np.abs(bank).max(axis=1)
        assert keep.any()
        with hc.Device(emu_library, N, prec) as dev:
            W = hc.run_hop(dev, x, kind, param, sj, hop)
        if prec == 64:                            # (the float32 signal is not a pure tone: its reference is the oracle's transform of it)
            assert hc.row_error(W[keep], closed[keep].astype(np.complex128), peak[keep]) <= hc.HOP_BOUND[prec]
        assert hc.row_error(W[keep], ref_full[keep][:, ::hop], peak[keep]) <= hc.HOP_BOUND[prec]


# ---- strides, batch, spectrum -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("output", [0, 1, 2])
def test_strides_sentinels_batch_and_spectrum(emu_library, prec, output):
    """ld > ncols_h and rows not asked for keep a sentinel's bits; x_ld > n0 with NaN padding; a batch of 3 is bit-identical to
    three single calls; the from-spectrum export is bit-identical to the from-signal one."""
    logn, hop, kind, param = 12, 16, orc.DOG, 2
    N, n0, nb = 1 << logn, (1 << logn) - 77, 3
    nch, pad = -(-n0 // hop), 5
    sj = hc.scales(N, kind, param)
    rows = len(sj)
    real, cplx = hc.types(prec)
    out_t = real if output == 1 else cplx
    sentinel = np.array([-7.0 if output == 1 else -7.0 - 7.0j], dtype=out_t)
    X = np.full((nb, n0 + 9), np.nan, dtype=real)
    X[:, :n0] = np.random.default_rng(8).standard_normal((nb, n0))
    Q = draw_q(12, (nb * rows + 2, nch + pad), real) if output == 2 else None
    with hc.Device(emu_library, N, prec, max_rows=nb * rows) as dev:
        xd = dev.up(X)
        out = dev.up(np.full((nb * rows + 2, nch + pad), sentinel[0], dtype=out_t))
        xh = dev.up(np.zeros((nb, N), dtype=cplx))
        qd = dev.up(Q) if Q is not None else None
        dev.plan.transform_hop(xd.ptr, nb, n0 + 9, n0, kind, param, 1.0, sj, hop, xh.ptr, output, out.ptr, nch + pad,
                               qd.ptr if qd else None, -0.75)
        full = out.download(dev.plan, (nb * rows + 2, nch + pad), out_t)
        sb = sentinel.view(np.uint8)
        assert np.all(np.ascontiguousarray(full[:nb * rows, nch:]).view(np.uint8).reshape(-1, sb.size) == sb)
        assert np.all(np.ascontiguousarray(full[nb * rows:]).view(np.uint8).reshape(-1, sb.size) == sb)
        assert not np.isnan(full[:nb * rows, :nch]).any()
        spectra = xh.download(dev.plan, (nb, N), cplx)
        for b in range(nb):                          # single calls: the same bits
            one = hc.run_hop(dev, X[b, :n0], kind, param, sj, hop, output=output, alpha=-0.75,
                             Q=None if Q is None else Q[b * rows:(b + 1) * rows, :nch])
            assert np.array_equal(one.view(np.uint8), np.ascontiguousarray(full[b * rows:(b + 1) * rows, :nch]).view(np.uint8)), b
        if output != 2:                              # from the spectra, batch stride > nfft
            wide = np.zeros((nb, N + 3), dtype=cplx)
            wide[:, :N] = spectra
            sd, o2 = dev.up(wide), dev.up(np.zeros((nb * rows, nch), dtype=out_t))
            dev.plan.transform_rows_hop(sd.ptr, nb, N + 3, n0, kind, param, 1.0, sj, hop, output, o2.ptr, nch)
            again = o2.download(dev.plan, (nb * rows, nch), out_t)
            assert np.array_equal(again.view(np.uint8), np.ascontiguousarray(full[:nb * rows, :nch]).view(np.uint8))
        if qd:
            assert np.array_equal(qd.download(dev.plan, Q.shape, real).view(np.uint8), Q.view(np.uint8))       # Q is never written


def test_non_finite_sample_gives_all_nan_rows(emu_library):
    N, n0, hop = 1 << 12, 4000, 16
    sj = hc.scales(N, orc.MORLET, 6)
    x = np.random.default_rng(2).standard_normal(n0)
    x[1234] = np.inf
    with hc.Device(emu_library, N, 64) as dev:
        assert np.isnan(hc.run_hop(dev, x, orc.MORLET, 6, sj, hop)).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(emu_library):
    """Every refusal of cwt_hip.h returns CWT_EINVAL with an empty launch log; M = 8192 is refused."""
    lib = emu_library
    dll = lib.dll
    N, n0, hop = 1 << 12, 4000, 16
    nch = -(-n0 // hop)
    sj = np.ascontiguousarray(hc.scales(N, orc.MORLET, 6))
    rows = len(sj)
    sp = sj.ctypes.data_as(C.POINTER(C.c_double))
    with hc.Device(lib, N, 64, max_rows=rows) as dev, hc.Device(lib, 1 << 16, 64, max_rows=rows) as big:
        xd, xh = dev.up(np.zeros(n0)), dev.up(np.zeros(N, dtype=np.complex128))
        out, q = dev.up(np.zeros((rows, nch), dtype=np.complex128)), dev.up(np.zeros((rows, nch)))
        xb = dev.up(np.zeros(n0))
        P = C.c_void_p

        def hop_call(h=None, x=xd.ptr, s=sp, o=out.ptr, qq=q.ptr, output=0, hop_=hop, ld=nch, nc=nch, nbatch=1, plan=None):
            return dll.cwt_transform_hop(plan or dev.plan.h, P(x), nbatch, n0, n0, 0, 6.0, 1.0, s, rows, hop_, P(xh.ptr), output, P(o), P(qq),
                                         2.0, ld, nc)

        def rows_call(output=0, hop_=hop, ld=nch, nc=nch, s=xh.ptr, o=out.ptr):
            return dll.cwt_transform_rows_hop(dev.plan.h, P(s), 1, N, n0, 0, 6.0, 1.0, sp, rows, hop_, output, P(o), ld, nc)

        def adj_call(hop_=hop, ldg=nch, nc=nch, g=out.ptr, xbar=xb.ptr, xbar_ld=n0, nbatch=1):
            return dll.cwt_adjoint_rows_hop(dev.plan.h, P(g), nbatch, rows * nch, ldg, nc, hop_, n0, 0, 6.0, 1.0, sp, rows, P(xbar), xbar_ld, 0)
        dev.plan.sync()
        dll.hipemu_clear_launched()
        refused = [
            ("hop not a power of two", hop_call(hop_=12, nc=-(-n0 // 12), ld=400)), ("hop < 2", hop_call(hop_=1, nc=n0, ld=n0)),
            ("hop = 0", hop_call(hop_=0)), ("M < 16", hop_call(hop_=512, nc=-(-n0 // 512))), ("ncols_h", hop_call(nc=nch - 1)),
            ("ncols_h too large", hop_call(nc=nch + 1, ld=nch + 1)), ("ld < ncols_h", hop_call(ld=nch - 1)),
            ("x NULL", hop_call(x=None)), ("scales NULL", hop_call(s=None)), ("out NULL", hop_call(o=None)),
            ("Q NULL", hop_call(output=2, qq=None)), ("Q overlaps the output", hop_call(output=2, qq=out.ptr)),
            ("Q's end on the output's start", hop_call(output=2, qq=out.ptr - (rows * nch - 1) * 8)),
            ("output 3", hop_call(output=3)), ("rows > max_rows", hop_call(nbatch=2)),
            ("M = 8192", hop_call(hop_=8, nc=-(-n0 // 8), ld=-(-n0 // 8), plan=big.plan.h)),
            ("spectrum NULL", rows_call(s=None)), ("weighted from a spectrum", rows_call(output=2)), ("rows: hop", rows_call(hop_=24)),
            ("rows: ld", rows_call(ld=nch - 1)), ("rows: ncols_h", rows_call(nc=nch + 1, ld=nch + 1)), ("rows: out NULL", rows_call(o=None)),
            ("adjoint: hop", adj_call(hop_=3)), ("adjoint: M", adj_call(hop_=1024, nc=-(-n0 // 1024))), ("adjoint: ncols_h", adj_call(nc=nch - 1)),
            ("adjoint: ldg", adj_call(ldg=nch - 1)), ("adjoint: G NULL", adj_call(g=None)), ("adjoint: xbar NULL", adj_call(xbar=None)),
            ("adjoint: xbar_ld", adj_call(xbar_ld=n0 - 1)), ("adjoint: rows > max_rows", adj_call(nbatch=2)),
        ]
        for name, rc in refused:
            assert rc == EINVAL and lib.cwt_last_error(), name
        assert launch_log(lib) == set()
        assert hop_call() == 0 and any("hop_rows" in s for s in launch_log(lib))          # ... and the good call goes through
    with pytest.raises(ValueError, match="power of two"):
        pycwt_amd.cwt_power(np.zeros(100), 1.0, hop=3)
    with pytest.raises(ValueError, match=r"\[16, 4096\]"):
        pycwt_amd.cwt_power(np.zeros(100), 1.0, hop=16)
    with pytest.raises(ValueError, match="pad"):
        pycwt_amd.cwt_power(np.zeros(100), 1.0, hop=4, pad=False)


# ---- the Python functions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", ["morlet", "paul", "dog"])
def test_python_functions_with_hop(emulated, wavelet):
    """cwt_power with hop=h: ceil(n0 / h) columns equal to columns ::h of the call
    without it (HOP_BOUND on W; on the power twice that, d|W|^2 = 2 |W| d|W|, plus the 4 eps of the square), coi[::h], sj and
    freqs unchanged, Paul's dropped rows as without hop."""
    n0, hop = 4019, 16
    x = np.random.default_rng(6).standard_normal(n0)
    P, sj, freqs, coi, fft5, fftfreqs = pycwt_amd.cwt_power(x, 0.25, 1 / 2, wavelet=wavelet)
    Ph, sjh, freqsh, coih, fft5h, fftfreqsh = pycwt_amd.cwt_power(x, 0.25, 1 / 2, wavelet=wavelet, hop=hop)
    assert Ph.shape == (len(sj), -(-n0 // hop)) and Ph.dtype == np.float64
    for a, b in ((sj, sjh), (freqs, freqsh), (coi[::hop], coih), (fftfreqs, fftfreqsh)):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(fft5h, fft5, rtol=0, atol=1e-13 * np.abs(fft5).max())
    bound = hc.power_slice_bound(64)
    peak = P.max(axis=1, keepdims=True)
    assert (np.abs(Ph - P[:, ::hop]) / peak).max() <= bound


def _device_results(x, wavelet, hop):
    dp = pycwt_amd.cwt_power_device(x, 0.25, 1 / 2, wavelet=wavelet, hop=hop)
    dw = pycwt_amd.cwt_device(x, 0.25, 1 / 2, wavelet=wavelet, hop=hop)
    try:
        return dp.power(), dw.W(), dp.coi, dw.coi, dp.shape, dw.shape, dp.global_power()
    finally:
        dp.close()
        dw.close()


@pytest.mark.parametrize("wavelet", ["morlet", "dog"])
def test_device_results_and_batch_with_hop(emulated, wavelet):
    n0, hop = 4019, 16
    rng = np.random.default_rng(16)
    x = rng.standard_normal(n0)
    Ph = pycwt_amd.cwt_power(x, 0.25, 1 / 2, wavelet=wavelet, hop=hop)
    P, W, coi_p, coi_w, shape_p, shape_w, gp = _device_results(x, wavelet, hop)
    assert shape_p == shape_w == Ph[0].shape and np.array_equal(coi_p, Ph[3]) and np.array_equal(coi_w, Ph[3])
    assert np.array_equal(P, Ph[0])                                        # the same export on the same plan
    Wd = W.astype(np.complex128)
    assert np.all(np.abs(P - (Wd.real ** 2 + Wd.imag ** 2)) <= 4 * np.finfo(np.float64).eps * P)
    np.testing.assert_allclose(gp, P.mean(axis=1), rtol=1e-12)
    X = rng.standard_normal((3, n0))
    X[0] = x
    Pb, sjb, _, coib, fftb, _ = pycwt_amd.cwt_power_batch(X, 0.25, 1 / 2, wavelet=wavelet, hop=hop)
    assert Pb.shape == (3,) + Ph[0].shape and np.array_equal(coib, Ph[3]) and np.array_equal(sjb, Ph[1])
    assert np.array_equal(Pb[0], Ph[0])                                    # a signal's bits do not depend on the batch


def test_state_does_not_leak(emulated, monkeypatch):
    """cwt, cwt_power and cwt_torch give the same bits before and after hop calls on the same plans: the cached row table is
    shared (no rebuild) and nothing of the hop call stays behind."""
    torch = pytest.importorskip("torch")
    from pycwt_amd import autograd, wavelet
    monkeypatch.setattr(autograd, "_engines", {})
    n0 = (1 << 16) - 5
    xn = np.random.default_rng(35).standard_normal(n0)
    xt = torch.as_tensor(xn)

    def all_three():
        return (pycwt_amd.cwt(xn, 1.0, 1 / 2)[0], pycwt_amd.cwt_power(xn, 1.0, 1 / 2)[0],
                pycwt_amd.cwt_torch(xt, 1.0, 1 / 2)[0].numpy().copy())
    before = all_three()
    pycwt_amd.cwt_power(xn, 1.0, 1 / 2, hop=16)
    x = xt.clone().requires_grad_(True)
    pycwt_amd.cwt_power_torch(x, 1.0, 1 / 2, hop=16)[0].sum().backward()
    y = xt.clone().requires_grad_(True)
    pycwt_amd.cwt_torch(y, 1.0, 1 / 2, hop=16)[0].abs().sum().backward()
    after = all_three()
    assert len(autograd._engines) == 1 and len(wavelet._plans) == 1
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    for eng in autograd._engines.values():
        eng.plan.close()


def test_hop_uses_the_cached_row_table_of_cwt_transform(emu_library):
    """after cwt_transform, a hop call of the same scales classifies nothing: no table kernels, only the hop kernels"""
    logn, hop, n0, kind, param = 16, 16, (1 << 16) - 77, orc.MORLET, 6
    sj = hc.scales(1 << logn, kind, param)
    x = hc.signal(n0, 64)
    with hc.Device(emu_library, 1 << logn, 64, options={"ols_min_logn": 15, "poly_min_logn": 14}) as dev:
        hc.run_full(dev, x, kind, param, sj)
        split = dev.plan.last_split()
        emu_library.dll.hipemu_clear_launched()
        hc.run_hop(dev, x, kind, param, sj, hop)
        log = launch_log(emu_library)
        assert not any("gtab" in s or "rtab" in s for s in log), log
        assert any("hop_fold" in s for s in log) and any("hop_rows" in s for s in log)
        assert dev.plan.last_split() == split


# ---- adjoint ----------------------------------------------------------------------------------------------------------------------
def run_adjoint(dev, G, n0, hop, kind, param, sj, onto=None, ldg=None):
    G = np.asarray(G)
    nb, rows, nch = G.shape
    ldg = nch if ldg is None else ldg
    Gp = np.full((nb, rows, ldg), np.nan + 0j, dtype=dev.cplx)
    Gp[:, :, :nch] = G
    gd = dev.up(Gp)
    xb = dev.up(np.zeros((nb, n0), dtype=dev.real) if onto is None else np.asarray(onto, dtype=dev.real))
    dev.plan.adjoint_rows_hop(gd.ptr, nb, rows * ldg, ldg, hop, n0, kind, param, 1.0, sj, xb.ptr, n0, onto is not None)
    return xb.download(dev.plan, (nb, n0), dev.real)


def dense_hop_operator(n0, N, hop, sj, m):
    """A_h (rows x ncols_h x n0), column by column from the oracle: column i = the oracle's rows of the unit vector e_i at ::hop"""
    nch = -(-n0 // hop)
    A = np.empty((len(sj), nch, n0), dtype=np.complex128)
    for i in range(n0):
        e = np.zeros(n0)
        e[i] = 1.0
        A[:, :, i] = orc.cwt_rows(e, 1.0, sj, m, N=N, intended=True)[:, :n0:hop]
    return A


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind,param", [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2)])
@pytest.mark.parametrize("hop", [4, 64])
def test_adjoint_against_the_dense_operator(emu_library, hop, kind, param, prec):
    """nfft = 2^10, n0 < nfft: Re(A_h^H G) of the dense operator; accumulate = 1; a batch bit-identical to single calls; a padded
    ldg.  Relative L2 within the bound of test_adjoint_emulated (1e-12 / 1e-5): the chain of roundings is that of
    cwt_adjoint_rows with a shorter first transform."""
    N, n0 = 1 << 10, 1000 - 13
    m = orc.Mother(kind, param)
    sj = hc.scales(N, kind, param, 8)
    A = dense_hop_operator(n0, N, hop, sj, m)
    rng = np.random.default_rng(21)
    nch = A.shape[1]
    G = random_g(rng, 3, len(sj), nch).astype(hc.types(prec)[1])
    want = np.real(np.einsum("jmn,bjm->bn", np.conj(A), G.astype(np.complex128)))
    with hc.Device(emu_library, N, prec) as dev:
        got = run_adjoint(dev, G, n0, hop, kind, param, sj, ldg=nch + 3)
        assert rel(got.astype(np.float64), want) <= ADJOINT_BOUND[prec]
        for b in range(3):
            one = run_adjoint(dev, G[b:b + 1], n0, hop, kind, param, sj)
            assert np.array_equal(one[0].view(np.uint8), got[b].view(np.uint8)), b
        base = rng.standard_normal((3, n0)).astype(dev.real)
        summed = run_adjoint(dev, G, n0, hop, kind, param, sj, onto=base)
        assert np.array_equal(summed, base + got)


@pytest.mark.parametrize("prec", PRECS)
def test_adjoint_identity_with_every_row_form_in_the_table(emu_library, prec):
    """2^15, hop = 16, the undecimated table holding every row form (FORMS_OPTS): Re <G, A_h x> = <x, A_h^H G> with A_h x from
    cwt_transform_hop, within hop_common.identity_bound (twice the relative-L2 bound of test_adjoint_emulated) of the scale."""
    N, n0, hop, kind, param = 1 << 15, (1 << 15) - 77, 16, orc.MORLET, 6
    sj = hc.scales(N, kind, param, 48)
    rng = np.random.default_rng(22)
    x = rng.standard_normal(n0)
    with hc.Device(emu_library, N, prec, options=dict(FORMS_OPTS)) as dev:
        hc.run_full(dev, x, kind, param, sj)
        kinds = {c.split("/")[0] for c in dev.plan.row_classes()}
        assert {"poly", "ols", "aols"} <= kinds and {"narrow", "two_pass", "narrow_k2048"} & kinds, kinds
        Ax = hc.run_hop(dev, x, kind, param, sj, hop).astype(np.complex128)
        G = random_g(rng, 1, *Ax.shape).astype(dev.cplx)
        xbar = run_adjoint(dev, G, n0, hop, kind, param, sj)[0].astype(np.float64)
    lhs = float(np.real(np.vdot(G[0].astype(np.complex128), Ax)))
    rhs = float(np.dot(x.astype(dev.real).astype(np.float64), xbar))
    scale = max(np.linalg.norm(G) * np.linalg.norm(Ax), np.linalg.norm(x) * np.linalg.norm(xbar))
    print("adjoint identity, precision", prec, ":", abs(lhs - rhs) / scale, "bound", hc.identity_bound(ADJOINT_BOUND, prec))
    assert abs(lhs - rhs) <= hc.identity_bound(ADJOINT_BOUND, prec) * scale, (lhs, rhs)


# ---- torch ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fresh_engines(emulated, monkeypatch):
    from pycwt_amd import autograd
    monkeypatch.setattr(autograd, "_engines", {})
    yield autograd
    for eng in autograd._engines.values():
        eng.plan.close()


@pytest.mark.parametrize("shape", [(131,), (2, 129)])
def test_gradcheck_with_hop(fresh_engines, shape):
    """nfft = 2^8, hop = 4, fp64: cwt_torch(hop=) of a signal, cwt_power_torch(hop=) of a signal and of a batch (dj = 2: a handful
    of rows keeps the dense Jacobians of gradcheck at a few hundred calls)"""
    torch = pytest.importorskip("torch")
    x = torch.randn(shape, dtype=torch.float64, requires_grad=True)
    if len(shape) == 1:
        assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_torch(t, 0.5, 2.0, wavelet="morlet", hop=4)[0], (x,), atol=1e-8)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 2.0, wavelet="dog", hop=4)[0], (x,), atol=1e-8)


@pytest.mark.parametrize("prec", PRECS)
def test_torch_values_and_gradient_against_the_existing_route(fresh_engines, prec):
    """cwt_torch(hop=h) equals cwt_torch[:, ::h] (sum of the two measured errors against the oracle), cwt_power_torch(hop=h) is
    its square, coi is coi[::h]; the gradient of a loss on W[:, ::h] through cwt_torch(hop=h) against the float64 NumPy adjoint
    within GRAD_BOUND = 4 x the measured error of the existing cwt_torch + slice (profiles/hop_accuracy.txt); x alone is saved by
    cwt_power_torch(hop=)."""
    torch = pytest.importorskip("torch")
    real_t = torch.float64 if prec == 64 else torch.float32
    N, n0, hop = 1 << 15, (1 << 15) - 77, 16
    rng = np.random.default_rng(41)
    x0 = torch.as_tensor(rng.standard_normal(n0), dtype=real_t)
    m = pycwt_amd.Morlet(6)
    xa = x0.clone().requires_grad_(True)
    W, sj, freqs, coi = pycwt_amd.cwt_torch(xa, 1.0, 1 / 4, wavelet=m)
    xb = x0.clone().requires_grad_(True)
    Wh, sjh, freqsh, coih = pycwt_amd.cwt_torch(xb, 1.0, 1 / 4, wavelet=m, hop=hop)
    nch = -(-n0 // hop)
    assert Wh.shape == (len(sj), nch) and Wh.dtype == W.dtype
    assert np.array_equal(sj, sjh) and np.array_equal(freqs, freqsh) and np.array_equal(coi[::hop], coih)
    Wn = W.detach().numpy().astype(np.complex128)
    peak = np.abs(Wn).max(axis=1)
    assert hc.row_error(Wh.detach().numpy(), Wn[:, ::hop], peak) <= hc.HOP_BOUND[prec] + hc.EXISTING_ERROR[prec]
    Cn = rng.standard_normal((len(sj), nch)) + 1j * rng.standard_normal((len(sj), nch))
    Ct = torch.as_tensor(Cn).to(W.dtype)
    (W[:, ::hop].conj() * Ct).real.sum().backward()
    (Wh.conj() * Ct).real.sum().backward()
    G = np.zeros((len(sj), n0), dtype=np.complex128)
    G[:, ::hop] = Ct.numpy().astype(np.complex128)
    bank = orc.filter_bank(np.asarray(sj, dtype=float), orc.angular_freqs(N, 1.0), N, orc.Mother(orc.MORLET, 6), True)
    ref = np.real(np.fft.ifft((np.conj(bank) * np.fft.fft(G, n=N, axis=1)).sum(axis=0)))[:n0]
    ea, eb = rel(xa.grad.numpy().astype(np.float64), ref), rel(xb.grad.numpy().astype(np.float64), ref)
    print("gradient against the NumPy adjoint, precision", prec, ": existing route", ea, "hop route", eb, "bound", hc.GRAD_BOUND[prec])
    assert xb.grad.dtype == real_t and eb <= hc.GRAD_BOUND[prec], (ea, eb)
    # the scalogram: values, what is saved, and its gradient against the route through cwt_torch(hop=)
    xc = x0.clone().requires_grad_(True)
    Ph, _, _, coip = pycwt_amd.cwt_power_torch(xc, 1.0, 1 / 4, wavelet=m, hop=hop)
    assert Ph.dtype == real_t and np.array_equal(coip, coih)
    Whn = Wh.detach().numpy().astype(np.complex128)
    want = Whn.real ** 2 + Whn.imag ** 2
    assert np.all(np.abs(Ph.detach().numpy().astype(np.float64) - want) <= 4 * np.finfo(hc.types(prec)[0]).eps * want)
    saved = Ph.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].shape == xc.shape
    gP = torch.as_tensor(rng.standard_normal(tuple(Ph.shape)), dtype=real_t)
    (Ph * gP).sum().backward()
    xd = x0.clone().requires_grad_(True)
    (pycwt_amd.cwt_torch(xd, 1.0, 1 / 4, wavelet=m, hop=hop)[0].abs().pow(2) * gP).sum().backward()
    assert rel(xc.grad.numpy().astype(np.float64), xd.grad.numpy().astype(np.float64)) <= ADJOINT_BOUND[prec]
    assert len(fresh_engines._engines) == 1


def test_lazily_conjugated_cotangent(fresh_engines):
    """The cotangent of `(W.conj() * C).real.sum()` taken on W itself reaches the backward with torch's conjugate bit set and its
    memory unconjugated; the backward resolves it, with and without hop: both gradients against the float64 NumPy adjoint of C
    (GRAD_BOUND; ignoring the bit gives the adjoint of conj(C), an error of order one)."""
    torch = pytest.importorskip("torch")
    N, n0, hop = 1 << 12, 4019, 16
    rng = np.random.default_rng(51)
    x0 = torch.as_tensor(rng.standard_normal(n0))
    bank = None
    for h in (None, hop):
        x = x0.clone().requires_grad_(True)
        W, sj, _, _ = pycwt_amd.cwt_torch(x, 1.0, 1 / 2, wavelet="morlet", hop=h)
        Cn = rng.standard_normal(tuple(W.shape)) + 1j * rng.standard_normal(tuple(W.shape))
        (W.conj() * torch.as_tensor(Cn)).real.sum().backward()
        G = np.zeros((len(sj), n0), dtype=np.complex128)
        G[:, ::(h or 1)] = Cn
        if bank is None:
            bank = orc.filter_bank(np.asarray(sj, dtype=float), orc.angular_freqs(N, 1.0), N, orc.Mother(orc.MORLET, 6), True)
        ref = np.real(np.fft.ifft((np.conj(bank) * np.fft.fft(G, n=N, axis=1)).sum(axis=0)))[:n0]
        assert rel(x.grad.numpy(), ref) <= hc.GRAD_BOUND[64], (h, rel(x.grad.numpy(), ref))


def test_batch_bits_do_not_depend_on_the_slabs(emulated):
    """cwt_power_batch(hop=) at nfft > 4096 under the automatic tolerance of the shim: a batch of 3 in one slab, in slabs of one
    signal, and each signal as a batch of its own give the same bits (the batch runs at the plan's tolerance, as without hop)."""
    n0, hop = 9000, 16
    X = np.random.default_rng(52).standard_normal((3, n0))
    pycwt_amd.set_tolerance("auto")
    whole = pycwt_amd.cwt_power_batch(X, 1.0, 1.0, wavelet="dog", hop=hop)[0]
    rows = whole.shape[1]
    slabs = pycwt_amd.cwt_power_batch(X, 1.0, 1.0, wavelet="dog", hop=hop, max_batch_bytes=rows * (-(-n0 // hop)) * 8)[0]
    assert np.array_equal(whole, slabs)
    for b in range(3):
        assert np.array_equal(pycwt_amd.cwt_power_batch(X[b:b + 1], 1.0, 1.0, wavelet="dog", hop=hop)[0][0], whole[b]), b


# ---- wavefront schedules (tests/emu/hipemu.cpp) -------------------------------------------------------------------------------------
LOCKSTEP, WAVES, WAVES_REVERSE, WAVES_SEEDED = 0, 1, 2, 3
WAVE_SCHEDULES = [("waves", WAVES, 0), ("waves-reverse", WAVES_REVERSE, 0), ("waves-seeded:1", WAVES_SEEDED, 1)]
HOP_KERNELS = {"hop_fold", "hop_rows", "hop_adj_accum"}


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


def schedule_case(lib, logn, hop, prec, fuse):
    """forward (W, power, weighted) and adjoint of one geometry: every hop kernel, as bytes"""
    N = 1 << logn
    n0, kind, param = N - 77, orc.DOG, 2
    sj = hc.scales(N, kind, param, 6)
    x = hc.signal(n0, prec, seed=9)
    with hc.Device(lib, N, prec, options={"hop_fuse_terms": fuse}) as dev:
        W = hc.run_hop(dev, x, kind, param, sj, hop)
        P = hc.run_hop(dev, x, kind, param, sj, hop, output=1)
        G = hc.run_hop(dev, x, kind, param, sj, hop, output=2, Q=draw_q(3, W.shape, dev.real), alpha=2.0)
        xbar = run_adjoint(dev, W[None], n0, hop, kind, param, sj)
    return [a.view(np.uint8).copy() for a in (W, P, G, xbar)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("logn,hop", [(12, 256), (12, 32), (12, 16), (12, 4), (12, 2), (16, 16)], ids=lambda v: str(v))
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, logn, hop, prec):
    """A race-free kernel cannot tell legal thread orders apart: forward, reverse and seeded wavefront orders give the bits of
    the lockstep order, for the fold kernel (LDS reduction over the runs of aliases), the transform kernel at M = 16 ... 4096
    (the run-time engine below 256 points, the wave-local and the workgroup-barrier instances of the compile-time engine above)
    and the adjoint's kernels.  test_emu_schedules.py's coverage gate lists the kernels named k_*; the hop kernels are gated
    here: each of them is launched under every schedule."""
    schedule(LOCKSTEP)
    base = schedule_case(emu_library, logn, hop, prec, 1)
    for label, k, s in WAVE_SCHEDULES:
        schedule(k, s)
        emu_library.dll.hipemu_clear_launched()
        got = schedule_case(emu_library, logn, hop, prec, 1)
        log = launch_log(emu_library)
        assert all(any(name in s for s in log) for name in HOP_KERNELS), (label, log)
        for a, b in zip(base, got):
            assert np.array_equal(a, b), label


def test_every_hop_kernel_is_known_to_the_schedule_test():
    """the kernels of cwt_kernels_hop.hpp are exactly those the schedule test launches"""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_hop.hpp")).read()
    assert set(re.findall(r"__global__[^{;]*?\b(hop_\w+)\s*\(", text)) == HOP_KERNELS
