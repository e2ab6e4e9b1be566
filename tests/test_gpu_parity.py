"""Parity tests proper: the HIP path on a real MI355X, called through the C ABI, against the oracle
and the reference-generated fixtures.  Run with `pytest -m gpu`.

Bars (BASELINE.json north_star): fp64 1e-6, fp32 1e-3 on per-row max|dW|/max|Wref|.  The asserted
tolerances below are tighter (1e-11 / 3e-5) because the engine is expected to be round-off exact.
"""
import numpy as np
import pytest

import pycwt_amd
from conftest import load_golden, row_errors
from oracle import cwt_oracle as orc
from pycwt_amd import _hip

pytestmark = pytest.mark.gpu
TOL = {64: 1e-11, 32: 3e-5}
MOTHERS = {"morlet": (orc.MORLET, 6), "paul": (orc.PAUL, 4), "dog": (orc.DOG, 2)}


def grid(n0, dt, mother, rows):
    s0 = 2 * dt / mother.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(n0 * dt / s0) / max(rows - 1, 1))
    return sj[~orc.dropped_rows(sj, dt, mother)]


def check_tuple(out, g, tol):
    W, sj, freqs, coi, fft, fftfreqs = out
    assert W.shape == g["W"].shape and W.dtype == np.complex128
    per_row, l2 = row_errors(W, g["W"])
    assert per_row.max() < tol and l2 < tol, (per_row.max(), l2)
    np.testing.assert_allclose(sj, g["sj"], rtol=1e-15)
    np.testing.assert_allclose(freqs, g["freqs"], rtol=1e-15)
    np.testing.assert_allclose(coi, g["coi"], rtol=1e-15)
    np.testing.assert_allclose(fft, g["fft"], rtol=0, atol=tol * np.abs(g["fft"]).max())


def test_backend_is_hip(hip_library):
    assert hip_library.backend() == "hip-gfx950" and hip_library.device_count() >= 1


def test_nino3_golden_through_shim(hip_library):
    g = load_golden("nino3_simple")
    out = pycwt_amd.cwt(g["x"], 0.25, 1 / 12, 0.5, 84, pycwt_amd.Morlet(6))
    check_tuple(out, g, TOL[64])
    W = out[0]
    assert abs(W[42, 252] - (-0.5998903691900097 - 0.9977145969302366j)) < 1e-11
    assert abs((np.abs(W) ** 2).sum() - 90362.0554906526) < 1e-5
    iw = pycwt_amd.icwt(W, out[1], 0.25, 1 / 12, pycwt_amd.Morlet(6))
    assert iw.dtype == np.complex128
    np.testing.assert_allclose(iw, g["icwt"], rtol=1e-10, atol=1e-11)
    out2 = pycwt_amd.cwt(load_golden("nino3_default")["x"], 0.25, wavelet="morlet")
    check_tuple(out2, load_golden("nino3_default"), TOL[64])


@pytest.mark.parametrize("name", ["mauna", "monsoon", "sunspot", "soi"])
def test_reference_sample_datasets_on_gpu(hip_library, name):
    """sample/sample.py's recipe on the reference's other datasets (sample/dataset.py:68-135), fixtures from the
    unmodified reference (every third row of W kept)."""
    g = load_golden("sample_" + name)
    W, sj, freqs, coi, fft, fftfreqs = pycwt_amd.cwt(g["x"], float(g["dt"]), 1 / 12, -1, -1, pycwt_amd.Morlet(6))
    assert W.shape == (int(g["nrows"]), g["x"].size)
    per_row, l2 = row_errors(W[g["rows"]], g["W"])
    assert per_row.max() < TOL[64] and l2 < TOL[64]
    np.testing.assert_allclose(sj, g["sj"], rtol=1e-14)
    np.testing.assert_allclose(coi, g["coi"], rtol=1e-14)
    np.testing.assert_allclose(fft, g["fft"], rtol=0, atol=TOL[64] * np.abs(g["fft"]).max())
    np.testing.assert_allclose(pycwt_amd.icwt(W, sj, float(g["dt"]), 1 / 12, pycwt_amd.Morlet(6)), g["icwt"], rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("name", ["morlet", "paul", "dog"])
def test_small_golden_all_mothers(hip_library, name):
    g = load_golden("small_" + name)
    out = pycwt_amd.cwt(g["x"], 0.5, 0.25, -1, -1, name)
    check_tuple(out, g, TOL[64])
    iw = pycwt_amd.icwt(out[0], out[1], 0.5, 0.25, name)
    assert iw.dtype == g["icwt"].dtype
    np.testing.assert_allclose(iw, g["icwt"], rtol=1e-10, atol=1e-11)
    out32 = pycwt_amd.cwt(g["x"], 0.5, 0.25, -1, -1, name, precision=32)
    per_row, l2 = row_errors(out32[0], g["W"])
    assert per_row.max() < 1e-3 and l2 < 1e-4


@pytest.mark.parametrize("name", ["morlet", "paul", "dog"])
def test_mid_golden_two_pass(hip_library, name):
    g = load_golden("mid_" + name)
    x = np.random.default_rng(int(g["seed"])).standard_normal(int(g["N"]))
    kind, param = MOTHERS[name]
    for opts in (None, {"narrow": 0}, {"chunk_rows": 1}, {"wg_points": 4096}, {"lmax": 256},
                 {"narrow": 0, "chunk_rows": 2}, {"overlap_narrow": 1}, {"ct": 0}):
        plan = _hip.Plan(int(g["N"]), 64, max_rows=32, options=opts)
        W, _ = plan.execute_host(x, kind, param, 1.0, g["sj"])
        plan.close()
        per_row, l2 = row_errors(W, g["W"])
        assert per_row.max() < TOL[64], (opts, per_row.max())


@pytest.mark.parametrize("N", [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                               65536, 1 << 18])
@pytest.mark.parametrize("prec", [64, 32])
def test_all_lengths_against_oracle(hip_library, N, prec):
    if N == 2:
        pytest.skip("reference yields NaN for N = 2")
    n0 = N if N < 64 else N - 3                         # ragged: zero padding + trimmed output
    x = np.random.default_rng(N).standard_normal(n0)
    for name, (kind, param) in MOTHERS.items():
        m = orc.Mother(kind, param)
        sj = grid(n0, 1.0, m, 9)
        plan = _hip.Plan(N, prec, max_rows=16)
        W, xhat = plan.execute_host(x, kind, param, 1.0, sj)
        plan.close()
        ref = orc.cwt_rows(x, 1.0, sj, m, N=N)[:, :n0]
        xref = np.fft.fft(x, n=N)
        assert np.abs(xhat - xref).max() / np.abs(xref).max() < TOL[prec]
        per_row, _ = row_errors(W, ref)
        assert per_row.max() < TOL[prec], (name, per_row.argmax(), per_row.max())


@pytest.mark.parametrize("name", ["morlet", "paul", "dog"])
def test_full_size_rows_against_reference_fixture(hip_library, name):
    """N = 2^20 on the 256-row grids of BASELINE configs 2/3: a row subset, compared with values the
    unmodified reference produced (tests/golden/big_*.npz: column samples + per-row norms)."""
    g = load_golden("big_" + name)
    N = int(g["N"])
    x = np.random.default_rng(int(g["seed"])).standard_normal(N)
    kind, param = MOTHERS[name]
    for prec in (64, 32):
        plan = _hip.Plan(N, prec, max_rows=16)
        W, _ = plan.execute_host(x, kind, param, 1.0, g["sj"], want_xhat=False)
        plan.close()
        err = np.abs(W[:, g["cols"]] - g["Wcols"]).max(axis=1) / g["rowmax"]
        assert err.max() < TOL[prec], (prec, err)
        np.testing.assert_allclose(np.abs(W).max(axis=1), g["rowmax"], rtol=10 * TOL[prec])
        np.testing.assert_allclose(np.sqrt((np.abs(W) ** 2).sum(axis=1)), g["rowl2"], rtol=10 * TOL[prec])
        assert (np.abs(W.sum(axis=1) - g["rowsum"]) < 1e3 * TOL[prec] * g["rowl2"]).all()


def _device_rows(plan, x, kind, param, sj, N):
    """Device-resident run: returns W (rows x N) as a host array."""
    xd = _hip.DeviceBuffer(x.nbytes)
    xh = _hip.DeviceBuffer(N * 16)
    Wd = _hip.DeviceBuffer(len(sj) * N * 16)
    xd.upload(plan, x)
    plan.forward_fft(xd.ptr, x.size, xh.ptr)
    plan.transform_rows(xh.ptr, kind, param, 1.0, sj, Wd.ptr, N, N)
    W = Wd.download(plan, (len(sj), N), np.complex128)
    for b in (xd, xh, Wd):
        b.free()
    return W


def test_full_size_properties_config2(hip_library):
    """Size-independent properties at N = 2^20 on all 256 scales of config 2 (rows in groups of 32):
    linearity, circular-shift covariance, cosine known answer (SURVEY 8c(2),(3))."""
    N = 1 << 20
    m = orc.Mother(orc.MORLET, 6)
    sj_all = grid(N, 1.0, m, 256)
    rng = np.random.default_rng(1234)
    x, y = rng.standard_normal(N), rng.standard_normal(N)
    mm = 12345
    wm = 2 * np.pi * mm / N
    n = np.arange(N)
    plan = _hip.Plan(N, 64, max_rows=256)
    for lo in range(0, 256, 64):
        sj = sj_all[lo:lo + 32]
        Wx = _device_rows(plan, x, orc.MORLET, 6, sj, N)
        Wy = _device_rows(plan, y, orc.MORLET, 6, sj, N)
        Wxy = _device_rows(plan, 2.0 * x - 0.5 * y, orc.MORLET, 6, sj, N)
        scale = np.abs(Wx).max(axis=1) + np.abs(Wy).max(axis=1)
        assert (np.abs(Wxy - (2.0 * Wx - 0.5 * Wy)).max(axis=1) / scale).max() < 1e-12
        del Wy, Wxy
        Ws = _device_rows(plan, np.roll(x, 4099), orc.MORLET, 6, sj, N)
        assert (np.abs(Ws - np.roll(Wx, 4099, axis=1)).max(axis=1) / scale).max() < 1e-12
        del Ws, Wx
        Wc = _device_rows(plan, np.cos(wm * n), orc.MORLET, 6, sj, N)
        pos = np.conj(m.psi_ft(sj * wm)) * np.sqrt(2 * np.pi * sj)
        neg = np.conj(m.psi_ft(-sj * wm)) * np.sqrt(2 * np.pi * sj)
        cols = np.r_[0:512, N - 512:N, 500000:500512]
        ref = 0.5 * (pos[:, None] * np.exp(1j * wm * cols) + neg[:, None] * np.exp(-1j * wm * cols))
        assert np.abs(Wc[:, cols] - ref).max() < 1e-10
        del Wc
    plan.close()


def test_icwt_device_path(hip_library):
    rng = np.random.default_rng(2)
    W = rng.standard_normal((40, 5000)) + 1j * rng.standard_normal((40, 5000))
    sj = 2.0 ** (np.arange(40) / 4)
    got = pycwt_amd.icwt(W, sj, 0.5, 0.25, "dog")
    ref = orc.icwt(W, sj, 0.5, 0.25, "dog")
    assert got.dtype == ref.dtype
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)


def test_edge_cases(hip_library):
    # single sample point more than a power of two -> padded to the next one; single scale; tiny dt
    x = np.random.default_rng(3).standard_normal(4097)
    out = pycwt_amd.cwt(x, 1e-3, freqs=np.array([7.0]), wavelet="morlet")
    ref = orc.cwt(x, 1e-3, freqs=np.array([7.0]), wavelet="morlet")
    assert out[0].shape == (1, 4097)
    per_row, _ = row_errors(out[0], ref[0])
    assert per_row.max() < TOL[64]
    # all-zero signal stays zero; constant signal has no NaN
    assert np.abs(pycwt_amd.cwt(np.zeros(300), 1.0)[0]).max() == 0
    assert np.isfinite(pycwt_amd.cwt(np.ones(300), 1.0, wavelet="paul")[0]).all()
    # scales far outside the resolvable range (empty filter support) give ~0 like the reference
    W = pycwt_amd.cwt(x, 1.0, freqs=np.array([1e-9, 0.2]), wavelet="dog")[0]
    Wr = orc.cwt_rows(x, 1.0, 1 / (orc.Mother(orc.DOG, 2).flambda() * np.array([1e-9, 0.2])),
                      orc.Mother(orc.DOG, 2))[:, :4097]
    assert W.shape == (2, 4097) and np.abs(W - Wr).max() < 1e-9


def test_sharded_api_single_rank_matches_cwt(hip_library):
    """parallel.cwt_sharded without a process group (1 GPU): device-resident shard == full transform."""
    import torch
    from pycwt_amd import parallel
    x = np.random.default_rng(8).standard_normal(3000)
    W, mine, sj, freqs, coi = parallel.cwt_sharded(x, 0.5, 0.25, wavelet="dog")
    ref = pycwt_amd.cwt(x, 0.5, 0.25, wavelet="dog")
    assert list(mine) == list(range(len(sj))) and W.is_cuda
    per_row, _ = row_errors(W.cpu().numpy(), ref[0])
    assert per_row.max() < 1e-12
    np.testing.assert_allclose(sj, ref[1])
    np.testing.assert_allclose(coi, ref[3])
    iw = parallel.icwt_sharded(W, sj[mine], 0.5, 0.25, "dog")
    np.testing.assert_allclose(iw, pycwt_amd.icwt(ref[0], ref[1], 0.5, 0.25, "dog"), rtol=1e-11, atol=1e-12)


def test_hip_engine_refuses_host_tensors(hip_library):
    """Tensors on the host would hand host pointers to the kernels (a GPU memory fault, not an error)."""
    from pycwt_amd import parallel
    with pytest.raises(RuntimeError, match="tensors on a GPU"):
        parallel.HipEngine(4096, 64, 8, 0, on_torch_stream=False)


@pytest.mark.parametrize("logn,prec,rows", [(21, 64, 6), (22, 64, 5), (23, 32, 4), (24, 32, 3), (24, 64, 2)])
def test_long_series_up_to_the_plan_limit(hip_library, logn, prec, rows):
    """N = 2^21 .. 2^24 (the two-pass limit lmax^2): column FFTs of 2048..4096 points, generic engine."""
    N = 1 << logn
    x = np.random.default_rng(logn).standard_normal(N - 7)
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, 1.0, m, rows)
    plan = _hip.Plan(N, prec, max_rows=8)
    W, xhat = plan.execute_host(x, orc.MORLET, 6, 1.0, sj)
    plan.close()
    ref = orc.cwt_rows(x, 1.0, sj, m, N=N)[:, :x.size]
    per_row, _ = row_errors(W, ref)
    assert per_row.max() < TOL[prec], per_row
    xref = np.fft.fft(x, n=N)
    assert np.abs(xhat - xref).max() / np.abs(xref).max() < TOL[prec]


def test_plan_rejects_lengths_beyond_limit(hip_library):
    with pytest.raises(_hip.HipError, match="power of two"):
        _hip.Plan(1 << 25, 64, max_rows=1)
    with pytest.raises(_hip.HipError, match="power of two"):
        _hip.Plan(3000, 64, max_rows=1)


# ---- callers of the hot path on the device ------------------------------
def test_callers_against_reference_fixture(hip_library):
    g = load_golden("callers")
    dt, dj, sj = float(g["dt"]), float(g["dj"]), g["sj"]
    m = pycwt_amd.Morlet(6)
    W12, coi, freq, signif = pycwt_amd.xwt(g["y1"], g["y2"], dt, dj, -1, -1, 0.95, m, True)
    assert np.abs(W12 - g["xwt_W12"]).max() < 1e-11 * np.abs(g["xwt_W12"]).max()
    np.testing.assert_allclose(signif, g["xwt_signif"], rtol=1e-12)
    W = pycwt_amd.cwt(g["y1"], dt, dj, -1, -1, m)[0]
    sc = m.smooth(W / sj[:, None], dt, dj, sj)
    assert np.abs(sc - g["smooth_complex"]).max() < 1e-12 * np.abs(g["smooth_complex"]).max()
    sr = m.smooth(np.abs(W) ** 2 / sj[:, None], dt, dj, sj)
    assert not np.iscomplexobj(sr) and np.abs(sr - g["smooth_real"]).max() < 1e-12 * np.abs(g["smooth_real"]).max()
    WCT, aWCT, coi, freq, sig = pycwt_amd.wct(g["y1"], g["y2"], dt, dj, -1, -1, False, 0.95, m, True)
    assert np.abs(WCT - g["wct"]).max() < 1e-10
    assert np.abs(np.angle(np.exp(1j * (aWCT - g["awct"])))).max() < 1e-9
    for prec, tol in ((32, 2e-3),):
        WCT32 = pycwt_amd.wct(g["y1"], g["y2"], dt, dj, sig=False, precision=prec)[0]
        assert np.abs(WCT32 - g["wct"]).max() < tol


def test_coherence_properties_long_series(hip_library):
    """N = 2^16: coherence of a series with itself is 1, with a scaled+delayed copy stays ~1 and the
    phase tracks the delay; smoothing on the two-pass/band-limited paths (per-row spectra)."""
    n = 1 << 16
    rng = np.random.default_rng(6)
    x = rng.standard_normal(n)
    WCT, aWCT, coi, freq, _ = pycwt_amd.wct(x, x, 1.0, 1.0, sig=False)
    assert np.abs(WCT - 1).max() < 1e-9 and np.abs(aWCT).max() < 1e-9
    y = 3.0 * np.roll(x, 5)
    WCT, aWCT, coi, freq, _ = pycwt_amd.wct(x, y, 1.0, 1.0, sig=False)
    inner = slice(n // 4, 3 * n // 4)
    assert WCT[6:, inner].min() > 0.97
    j = 8                                              # period = 1/freq[j]; a delay of 5 samples is a phase of 2*pi*5*f
    expect = 2 * np.pi * 5 * freq[j]
    assert abs(np.median(aWCT[j, inner]) - expect) < 0.05 * max(1.0, expect)


def test_wct_significance_gpu(hip_library, tmp_path, monkeypatch):
    from pycwt_amd import wavelet
    monkeypatch.setattr(wavelet, "get_cache_dir", lambda: str(tmp_path) + "/")
    np.random.seed(1)
    sig = pycwt_amd.wct_significance(0.6, 0.4, dt=0.5, dj=0.25, s0=1.0, J=20, mc_count=40, progress=False)
    ok = np.isfinite(sig)
    assert ok.sum() >= 10 and (sig[ok] > 0.5).all() and (sig[ok] < 1).all()
    # the 95 % coherence level of red noise grows only mildly with scale (Grinsted et al. 2004, fig. 3)
    assert sig[ok].max() - sig[ok].min() < 0.4


def test_wct_significance_seed_for_seed_with_the_reference_gpu(hip_library):
    from test_callers_emulated import _seeded_significance_cases
    _seeded_significance_cases()


@pytest.mark.parametrize("precision", [64, 32])
def test_coherence_histogram_gpu(hip_library, precision):
    from test_callers_emulated import _histogram_case
    _histogram_case(hip_library, precision)


@pytest.mark.parametrize("precision", [64, 32])
def test_boxcar_gpu(hip_library, precision):
    from test_callers_emulated import _boxcar_case
    _boxcar_case(hip_library, precision)


def test_custom_mother_objects_on_gpu(hip_library):
    """Duck-typed mothers go through the explicit filter-bank kernel (all three transform paths)."""
    import scipy.fft as sfft

    class Custom:
        name = "custom"
        def psi_ft(self, f):
            with np.errstate(all="ignore"):
                return (0.8 - 0.3j) * np.where(f > 0, np.abs(f) ** 1.5, 0.0) * np.exp(-0.5 * (f - 2.0) ** 2)
        def flambda(self): return 2.5
        def coi(self): return 1.1

    m = Custom()
    for n0, prec, tol in ((300, 64, 1e-12), (5000, 64, 1e-12), (70000, 64, 1e-12), (70000, 32, 3e-5)):
        x = np.random.default_rng(n0).standard_normal(n0)
        W, sj, *_ = pycwt_amd.cwt(x, 0.5, 0.5, wavelet=m, precision=prec)
        N = int(2 ** np.ceil(np.log2(n0)))
        w = 2 * np.pi * np.fft.fftfreq(N, 0.5)
        bank = (sj[:, None] * w[1] * N) ** .5 * np.conjugate(m.psi_ft(sj[:, None] * w))
        ref = sfft.ifft(sfft.fft(x, n=N) * bank, axis=1)[:, :n0]
        per_row, _ = row_errors(W, ref)
        assert per_row.max() < tol, (n0, prec, per_row.max())


def test_config4_shape_batch_of_signals(hip_library):
    """BASELINE config 4 at test size: signals of N = 2^16, Morlet, 128 scales, as one batched launch set;
    checked against the oracle on sampled rows and against the single-signal path; the sharded API
    (single rank) must agree too."""
    import time
    import torch
    from pycwt_amd import parallel
    nb, n0, rows = 6, 1 << 16, 128
    X = np.random.default_rng(1234).standard_normal((nb, n0))
    m = orc.Mother(orc.MORLET, 6)
    s0 = 2 / m.flambda()
    dj = np.log2(n0 / s0) / (rows - 1)
    t0 = time.perf_counter()
    Wb, sj, freqs, coi, fftb, _ = pycwt_amd.cwt_batch(X, 1.0, dj, s0, rows - 1, "morlet")
    t_batch = time.perf_counter() - t0
    assert Wb.shape == (nb, rows, n0)
    sel = [0, 31, 64, 100, 127]
    for b in (0, nb - 1):
        ref = orc.cwt_rows(X[b], 1.0, sj[sel], m)
        per_row, _ = row_errors(Wb[b, sel], ref)
        assert per_row.max() < TOL[64]
    W1 = pycwt_amd.cwt(X[2], 1.0, dj, s0, rows - 1, "morlet")[0]
    per_row, _ = row_errors(Wb[2], W1)
    assert per_row.max() < TOL[64]          # the batch takes the overlap-save form for its time-compact rows, one signal of 2^16 does not
    Wl, mine, sj2, _, _ = parallel.cwt_sharded(X, 1.0, dj, s0, rows - 1, "morlet")
    assert tuple(Wl.shape) == (nb, rows, n0)
    assert np.abs(Wl[3].cpu().numpy() - Wb[3]).max() == 0
    print(f"batch of {nb} x 2^16 x {rows}: {t_batch * 1e3:.1f} ms host wall incl. PCIe")


def test_device_resident_workflow_on_gpu(hip_library):
    """cwt_device + reductions (global spectrum, scale average, reconstruction) against NumPy on the
    downloaded matrix, N = 2^18 so that all three transform paths contribute rows."""
    n0 = (1 << 18) - 11
    x = np.random.default_rng(18).standard_normal(n0)
    dj = 0.25
    T = pycwt_amd.cwt_device(x, 1.0, dj, wavelet="morlet")
    W = T.W()
    ref = orc.cwt_rows(x, 1.0, T.sj[[0, 20, 40, 60]], orc.Mother(orc.MORLET, 6))[:, :n0]
    per_row, _ = row_errors(W[[0, 20, 40, 60]], ref)
    assert per_row.max() < TOL[64]
    power = np.abs(W) ** 2
    np.testing.assert_allclose(T.global_power(), power.mean(axis=1), rtol=1e-10)
    sel = (T.sj >= 4) & (T.sj < 64)
    np.testing.assert_allclose(T.scale_average(4, 64, dj), dj / 0.776 * (power / T.sj[:, None])[sel].sum(axis=0),
                               rtol=1e-10)
    np.testing.assert_allclose(T.icwt(dj), orc.icwt(W, T.sj, 1.0, dj, "morlet"), rtol=1e-10, atol=1e-11)
    T.close()


def test_config5_deterministic_part_at_full_size(hip_library):
    """BASELINE config 5 without the Monte-Carlo loop: xwt and wct of two N = 2^20 series on the device
    (per-row-spectrum smoothing through the band-limited and two-pass kernels).  Checked against NumPy on
    sampled scales (the smoothing of mothers.py:61-104 restated with scipy.fft on those rows only)."""
    import scipy.fft as sfft
    from pycwt_amd.helpers import rect
    n = 1 << 20
    rng = np.random.default_rng(55)
    e = rng.standard_normal(n)
    y1 = e + np.sin(2 * np.pi * np.arange(n) / 500.0)
    y2 = 0.5 * np.roll(e, 3) + rng.standard_normal(n) + np.sin(2 * np.pi * np.arange(n) / 500.0 + 0.7)
    dt, dj = 1.0, 0.5
    m = pycwt_amd.Morlet(6)
    WCT, aWCT, coi, freq, sig = pycwt_amd.wct(y1, y2, dt, dj, sig=False)
    rows = WCT.shape[0]
    assert WCT.shape == (rows, n) and np.isfinite(WCT).all() and WCT.min() >= 0 and WCT.max() <= 1 + 1e-9
    # reference for scale rows j0..j1 needs the boxcar neighbours: rebuild the unsmoothed inputs on a window of scales
    sj = 1 / (m.flambda() * freq)
    y1n, y2n = (y1 - y1.mean()) / y1.std(), (y2 - y2.mean()) / y2.std()
    win = rect(int(np.round(m.deltaj0 / dj * 2)), normalize=True)
    half = (len(win) - 1) // 2
    for j in (3, 17, rows - 4):
        lo, hi = max(0, j - half - 1), min(rows, j + half + 2)
        o = orc.Mother(orc.MORLET, 6)
        W1 = orc.cwt_rows(y1n, dt, sj[lo:hi], o)
        W2 = orc.cwt_rows(y2n, dt, sj[lo:hi], o)
        k2 = (2 * np.pi * np.fft.fftfreq(n)) ** 2
        def tsmooth(T):
            F = np.exp(-0.5 * (sj[lo:hi, None] / dt) ** 2 * k2)
            return sfft.ifft(F * sfft.fft(T, axis=1), axis=1)
        S1 = tsmooth(np.abs(W1) ** 2 / sj[lo:hi, None]).real
        S2 = tsmooth(np.abs(W2) ** 2 / sj[lo:hi, None]).real
        S12 = tsmooth(W1 * W2.conj() / sj[lo:hi, None])
        def box(T, jj):                                   # convolve2d(T, win[:, None], 'same') at row jj
            acc = 0
            for i, w in enumerate(win):
                r = jj + half - i
                if 0 <= r < rows:
                    acc = acc + w * T[r - lo]
            return acc
        ref = np.abs(box(S12, j)) ** 2 / (box(S1, j) * box(S2, j))
        assert np.abs(WCT[j] - ref).max() < 1e-9, j
        assert np.abs(np.angle(np.exp(1j * (aWCT[j] - np.angle(W1[j - lo] * W2[j - lo].conj()))))).max() < 1e-8
    W12, xcoi, xfreq, xsig = pycwt_amd.xwt(y1, y2, dt, dj)
    assert W12.shape == (rows, n)
    o = orc.Mother(orc.MORLET, 6)
    ref = orc.cwt_rows(y1n, dt, sj[[5]], o) * orc.cwt_rows(y2n, dt, sj[[5]], o).conj()
    assert np.abs(W12[5] - ref[0]).max() < 1e-10 * np.abs(ref).max()


def test_stream_overlap_options_keep_parity_at_full_size(hip_library):
    """The side-stream placement (band-limited rows beside the two-pass chain) and the chunking of the two-pass rows must
    not change a single bit."""
    N = 1 << 20
    x = np.random.default_rng(77).standard_normal(N)
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, 1.0, m, 256)[:160:4]                     # 40 rows, mostly two-pass
    base = None
    for opts in ({"overlap_narrow": 0}, None, {"chunk_rows": 3}, {"overlap_narrow": 1}, {"chunk_rows": 5}):
        plan = _hip.Plan(N, 64, max_rows=64, options=opts)
        for _ in range(3):                                # repeated calls re-use the two buffers
            W = _device_rows(plan, x, orc.MORLET, 6, sj, N)
        plan.close()
        if base is None:
            base = W
            ref = orc.cwt_rows(x, 1.0, sj[[0, 13, 39]], m)
            per_row, _ = row_errors(W[[0, 13, 39]], ref)
            assert per_row.max() < TOL[64]
        else:
            assert np.array_equal(W, base), opts


def test_fp32_band_limited_tile_variants_agree(hip_library):
    """complex64 band-limited rows: K <= 512 on half-size tiles (default) or on the 16384-point instance (narrow_small = 0,
    the one compiled for two workgroups per CU) -- the same arithmetic per output (bit-identical on the emulator; on the
    device the two instances may contract multiply-adds differently, hence a few ulp); and both within the fp32 tolerance
    of the oracle for every transform length K."""
    N = 1 << 20
    x = np.random.default_rng(78).standard_normal(N).astype(np.float32)
    m = orc.Mother(orc.MORLET, 6)
    sj = 3.04e6 / np.array([12.0, 24, 48, 100, 200, 400, 800, 1000, 1500, 2500])     # K = 16 ... 1024, then two terms
    out = {}
    for small in (1, 0):
        plan = _hip.Plan(N, 32, max_rows=16, options={"narrow_small": small, "poly": 0})   # (poly = 1 would take these rows)
        xd, xh, Wd = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 8), _hip.DeviceBuffer(len(sj) * N * 8)
        xd.upload(plan, x)
        plan.transform(xd.ptr, N, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
        out[small] = Wd.download(plan, (len(sj), N), np.complex64)
        labels = plan.row_classes()
        for b in (xd, xh, Wd):
            b.free()
        plan.close()
        assert all(l.startswith("narrow/") for l in labels), labels
    assert np.abs(out[0] - out[1]).max() <= 1e-6 * np.abs(out[1]).max()
    ref = orc.cwt_rows(x.astype(np.float64), 1.0, sj, m)
    per_row, _ = row_errors(out[1], ref)
    assert per_row.max() < TOL[32], per_row


def _download_rows(plan, buf, lo, cnt, ld, dtype):
    """Rows [lo, lo + cnt) of a device-resident row-major matrix with `ld` elements of `dtype` per row."""
    import ctypes as C
    out = np.empty((cnt, ld), dtype=dtype)
    plan.lib.check(plan.lib.cwt_memcpy_d2h(plan.h, out.ctypes.data_as(C.c_void_p),
                                           C.c_void_p(buf.ptr + lo * ld * out.itemsize), out.nbytes))
    return out


@pytest.mark.parametrize("target", ["round-off", "bench"])
@pytest.mark.parametrize("name,prec", [("morlet", 64), ("paul", 32), ("dog", 32), ("paul", 64), ("dog", 64)])
def test_every_row_of_the_bench_workloads_against_the_oracle(hip_library, name, prec, target):
    """BASELINE configs 2 and 3 exactly as bench.py times them -- N = 2^20, all 256 rows, device resident, through
    cwt_transform (forward FFT + rows, every row form) -- with EVERY row compared with the oracle (pycwt/wavelet.py:91-106
    restated), in slabs of 16 rows.  Prints the worst row per kernel class.  Rows the reference turns into NaN
    (Paul: 161 of 256, wavelet.py:111-115) have no reference value: they are compared with the "intended value" oracle
    (cwt_rows(..., intended=True): Heaviside before the exponential, identical to the reference on the rows it keeps).
    ("paul", 64) and ("dog", 64) are not BASELINE configs (config 3 is quoted in fp32) but the reference's own arithmetic
    for those mothers (mothers.py:118-122, 170-173 yield complex128) and what `pycwt_amd.cwt(..., 'paul')` runs by default.
    target "round-off": every truncation below the arithmetic's rounding (the suite's setting); "bench": the accuracy target
    bench.py times (bench.BENCH_TOLERANCE), i.e. the SAME row classification as the headline, against bench.py's own bar."""
    import bench
    N, rows = 1 << 20, 256
    kind, param = MOTHERS[name]
    m = orc.Mother(kind, param)
    s0 = 2 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))           # SURVEY 8d grid (no rows dropped)
    x = np.random.default_rng(1234).standard_normal(N)
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    x = x.astype(real)
    plan = _hip.Plan(N, prec, max_rows=rows, options={"tolerance": bench.BENCH_TOLERANCE[prec]} if target == "bench" else None)
    bar = bench.PARITY_TOL[prec] if target == "bench" else TOL[prec]
    xd, xh = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 2 * x.itemsize)
    Wd = _hip.DeviceBuffer(rows * N * 2 * x.itemsize)
    xd.upload(plan, x)
    plan.transform(xd.ptr, N, kind, param, 1.0, sj, xh.ptr, Wd.ptr, N, N)
    classes = plan.row_classes()
    assert len(classes) == rows
    assert any(c.startswith("poly/") for c in classes)
    if not (name == "paul" and prec == 64):          # (fp64 Paul at round-off: the 1/t^5 tail leaves no row a halo that fits a tile)
        assert any(c.startswith("ols/") for c in classes)
    if name != "dog" and prec == 32 or name == "morlet":
        assert any(c.startswith("aols/") for c in classes)
    dropped = orc.dropped_rows(sj, 1.0, m)
    worst, checked, n_intended = {}, 0, 0
    for lo in range(0, rows, 16):
        got = _download_rows(plan, Wd, lo, 16, N, cplx)
        assert np.isfinite(got.view(real)).all()
        with np.errstate(all="ignore"):
            ref = orc.cwt_rows(x, 1.0, sj[lo:lo + 16], m, intended=True)
        for k in range(16):
            j = lo + k
            err = np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()
            checked += not dropped[j]
            if dropped[j]:
                n_intended += 1
            if err >= worst.get(classes[j], (0.0, -1))[0]:
                worst[classes[j]] = (float(err), j)
    plan_tol = plan.tolerance()
    for b in (xd, xh, Wd):
        b.free()
    plan.close()
    print(f"{name} fp{prec} ({target}, tolerance {plan_tol:g}): {checked} rows compared with the reference's arithmetic, "
          f"{n_intended} (rows the reference drops) with the intended-value oracle; worst row per kernel class:")
    for c in sorted(worst):
        print(f"   {c:22s} row {worst[c][1]:3d}  err {worst[c][0]:.3e}")
    assert checked == rows - int(dropped.sum()) and checked >= 90      # Paul: 95 rows survive the reference's NaN rule
    assert max(v[0] for v in worst.values()) < bar, worst


def test_config4_full_batch_sampled_pairs(hip_library):
    """BASELINE config 4 at full size on one GPU: 1024 signals x N = 2^16 x 128 Morlet scales through ONE batched
    launch set (cwt_transform_batch: forward transforms, block spectra per signal, rows; 137 GB of W device resident),
    checked against the oracle on sampled (signal, scale) pairs that cover every kernel class of the row table."""
    nb, N, rows = 1024, 1 << 16, 128
    m = orc.Mother(orc.MORLET, 6)
    s0 = 2 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))
    X = np.random.default_rng(1234).standard_normal((nb, N))
    plan = _hip.Plan(N, 64, max_rows=nb * rows)
    xd, xh = _hip.DeviceBuffer(X.nbytes), _hip.DeviceBuffer(nb * N * 16)
    Wd = _hip.DeviceBuffer(nb * rows * N * 16)
    xd.upload(plan, X)
    plan.transform_batch(xd.ptr, nb, N, N, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
    plan.sync()
    classes = plan.row_classes()
    assert len(classes) == nb * rows
    assert any(c.startswith("ols") for c in classes) and any(c.startswith("aols") for c in classes)
    assert not any(c.startswith("two_pass") for c in classes)      # (round 3: 9 two-pass rows per signal)
    xhat0 = _download_rows(plan, xh, nb - 1, 1, N, np.complex128)[0]
    ref0 = np.fft.fft(X[nb - 1])
    assert np.abs(xhat0 - ref0).max() < 1e-12 * np.abs(ref0).max()
    rng = np.random.default_rng(7)
    pairs = {(0, 0), (nb - 1, rows - 1), (nb - 1, 0), (0, rows - 1)}
    for c in sorted(set(classes)):                       # two random pairs of every kernel class
        idx = np.flatnonzero(np.array(classes) == c)
        for i in rng.choice(idx, size=min(2, idx.size), replace=False):
            pairs.add((int(i) // rows, int(i) % rows))
    while len(pairs) < 48:
        pairs.add((int(rng.integers(nb)), int(rng.integers(rows))))
    # ... and 512 more drawn with a FRESH seed every run (printed, so that a failure can be replayed with CWT_TEST_SEED):
    # unlike Parseval on all rows (test_config4_full_batch_parseval_on_every_row) a sampled row sees a phase error
    import os
    seed = int(os.environ.get("CWT_TEST_SEED", np.random.SeedSequence().entropy % (1 << 32)))
    fresh = np.random.default_rng(seed)
    print(f"config 4 fresh pairs: CWT_TEST_SEED={seed}")
    while len(pairs) < 48 + 512:
        pairs.add((int(fresh.integers(nb)), int(fresh.integers(rows))))
    worst, where = 0.0, None
    for b, j in sorted(pairs):
        got = _download_rows(plan, Wd, b * rows + j, 1, N, np.complex128)[0]
        ref = orc.cwt_rows(X[b], 1.0, sj[j:j + 1], m)[0]
        err = np.abs(got - ref).max() / np.abs(ref).max()
        if err > worst:
            worst, where = err, (b, j, classes[b * rows + j])
    for buf in (xd, xh, Wd):
        buf.free()
    plan.close()
    print(f"config 4 full batch: {len(pairs)} (signal, scale) pairs, worst row error {worst:.3e} at {where}")
    assert worst < TOL[64], (seed, where, worst)


@pytest.mark.parametrize("precision,tol", [(64, 1e-11), (32, 2e-4)])
def test_unpadded_transform_lengths_on_gpu(hip_library, precision, tol):
    """pad=False (the reference's pyfftw branch, helpers.py:15-19): reference-generated fixture at n0 = 504 / 1000 / 331
    and the oracle at n0 = 65521 (prime) and 1 000 003."""
    g = load_golden("unpadded")
    for tag in "abc":
        out = pycwt_amd.cwt(g[f"{tag}_x"], 0.5, 1 / 4, -1, -1, str(g[f"{tag}_name"]), pad=False, precision=precision)
        per_row, l2 = row_errors(out[0], g[f"{tag}_W"])
        assert out[0].shape == g[f"{tag}_W"].shape and per_row.max() < tol and l2 < tol, (tag, per_row.max())
        np.testing.assert_allclose(out[4], g[f"{tag}_fft"], rtol=0, atol=tol * np.abs(g[f"{tag}_fft"]).max())
    for n0, dj in ((65521, 1.0), (1000003, 4.0)):
        x = np.random.default_rng(n0).standard_normal(n0)
        out = pycwt_amd.cwt(x, 1.0, dj, -1, -1, "morlet", pad=False, precision=precision)
        ref = orc.cwt(x.astype(np.float32) if precision == 32 else x, 1.0, dj, -1, -1, "morlet", pad=False)
        per_row, _ = row_errors(out[0], ref[0])
        assert out[0].shape == ref[0].shape and per_row.max() < tol, (n0, per_row.max())


@pytest.mark.parametrize("name,prec,logn,n0_off", [("morlet", 64, 18, 0), ("morlet", 64, 20, 12345), ("morlet", 32, 19, 7),
                                                   ("paul", 32, 20, 1), ("paul", 64, 17, 0), ("dog", 32, 20, 0),
                                                   ("dog", 64, 19, 4097)])
def test_overlap_save_rows_on_gpu(hip_library, name, prec, logn, n0_off):
    """cwt_transform (the signal is known: time-compact rows go block by block through k_ols_fwd / k_ols_ct, incl. the
    double-length blocks) against cwt_forward_fft + cwt_transform_rows (the same rows through the two-pass / band-limited
    kernels) on every row, against the oracle on a row sample, and bit for bit across the stream options."""
    N = 1 << logn
    n0 = N - n0_off
    kind, param = MOTHERS[name]
    m = orc.Mother(kind, param)
    sj = grid(n0, 1.0, m, 96)
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    x = np.random.default_rng(logn + n0_off).standard_normal(n0).astype(real)
    plan = _hip.Plan(N, prec, max_rows=len(sj), options={"ols_big": 1, "ols_min_logn": 15, "poly": 0})   # defaults: fp32 only, 2^18;
    # poly = 0: the rows with the longest halos would otherwise take the polynomial form
    xd, xh = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 2 * x.itemsize)
    Wa, Wb = (_hip.DeviceBuffer(len(sj) * n0 * 2 * x.itemsize) for _ in range(2))
    xd.upload(plan, x)
    plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wa.ptr, n0, n0)
    split, classes = plan.last_split(), plan.row_classes()
    if name == "paul" and prec == 64:      # polynomial tails: no halo reaches 1e-17 of the wavelet's mass -> never taken
        assert split["ols"] == 0
        for b in (xd, xh, Wa, Wb):
            b.free()
        plan.close()
        return
    assert split["ols"] >= 8, split
    if logn >= 18 and name != "paul":
        assert any(c.startswith("ols2/") for c in classes), sorted(set(classes))
    A = Wa.download(plan, (len(sj), n0), cplx)
    plan.forward_fft(xd.ptr, n0, xh.ptr)
    plan.transform_rows(xh.ptr, kind, param, 1.0, sj, Wb.ptr, n0, n0)
    assert plan.last_split()["ols"] == 0
    B = Wb.download(plan, (len(sj), n0), cplx)
    per_row, _ = row_errors(A, B)
    assert per_row.max() < TOL[prec], (per_row.argmax(), classes[per_row.argmax()], per_row.max())
    mine = [i for i, c in enumerate(classes) if c.startswith("ols")]
    pick = mine[::max(1, len(mine) // 6)]
    with np.errstate(all="ignore"):
        ref = orc.cwt_rows(x, 1.0, sj[pick], m, N=N)[:, :n0]
    per_row, _ = row_errors(A[pick], ref)
    assert per_row.max() < TOL[prec], (per_row, [classes[i] for i in pick])
    for opts in ({"ols_early": 0}, {"ols_early": 0, "ols_side": 0}, {"overlap_narrow": 0}):
        for k, v in opts.items():
            plan.set_option(k, v)
        plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wb.ptr, n0, n0)
        assert np.array_equal(Wb.download(plan, (len(sj), n0), cplx), A), opts
        for k in opts:
            plan.set_option(k, 1)
    plan.set_option("ols_big", 0)
    plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wb.ptr, n0, n0)
    per_row, _ = row_errors(Wb.download(plan, (len(sj), n0), cplx), A)
    assert per_row.max() < TOL[prec]
    plan.set_option("ols_small_max_halo", 0)            # every overlap-save row on the default tile
    plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wb.ptr, n0, n0)
    assert plan.last_split()["ols"] >= 8 and not any(c.endswith("/half") for c in plan.row_classes())
    per_row, _ = row_errors(Wb.download(plan, (len(sj), n0), cplx), A)
    assert per_row.max() < TOL[prec]
    for b in (xd, xh, Wa, Wb):
        b.free()
    plan.close()


@pytest.mark.parametrize("name,prec,logn,rows", [("morlet", 64, 21, 48), ("dog", 32, 23, 40), ("morlet", 64, 23, 32)])
def test_overlap_save_rows_of_long_series(hip_library, name, prec, logn, rows):
    """The overlap-save classes at N = 2^21 and 2^23 (more blocks per row, longer halos in samples, both tile sizes and
    the double-length blocks): EVERY such row of cwt_transform against the same row through cwt_forward_fft +
    cwt_transform_rows (N-point kernels), and one row of every class label against the oracle."""
    N = 1 << logn
    n0 = N - 4099
    kind, param = MOTHERS[name]
    m = orc.Mother(kind, param)
    sj = grid(n0, 1.0, m, rows)
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    x = np.random.default_rng(logn).standard_normal(n0).astype(real)
    plan = _hip.Plan(N, prec, max_rows=len(sj), options={"ols_big": 1, "poly": 0})
    xd, xh = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 2 * x.itemsize)
    Wa, Wb = (_hip.DeviceBuffer(len(sj) * n0 * 2 * x.itemsize) for _ in range(2))
    xd.upload(plan, x)
    plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wa.ptr, n0, n0)
    classes = plan.row_classes()
    mine = [i for i, c in enumerate(classes) if c.startswith("ols")]
    labels = sorted({classes[i] for i in mine})
    assert len(mine) >= rows // 4, labels
    assert any(c.endswith("/half") for c in labels) and any(c.startswith("ols/") and not c.endswith("/half") for c in labels), labels
    assert any(c.startswith("ols2/") for c in labels), labels
    plan.forward_fft(xd.ptr, n0, xh.ptr)
    plan.transform_rows(xh.ptr, kind, param, 1.0, sj, Wb.ptr, n0, n0)
    assert plan.last_split()["ols"] == 0
    es = 2 * x.itemsize
    worst = {}
    for i in mine:                                       # row by row: W is up to 4 GiB here
        a, b = np.empty(n0, cplx), np.empty(n0, cplx)
        for buf, out in ((Wa, a), (Wb, b)):
            plan.lib.check(plan.lib.cwt_memcpy_d2h(plan.h, out.ctypes.data, buf.ptr + i * n0 * es, out.nbytes))
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst[classes[i]] = max(worst.get(classes[i], 0.0), err)
        assert err < TOL[prec], (i, classes[i], err)
    pick = [next(i for i in mine if classes[i] == c) for c in labels]
    with np.errstate(all="ignore"):
        ref = orc.cwt_rows(x, 1.0, sj[pick], m, N=N)[:, :n0]
    for k, i in enumerate(pick):
        a = np.empty(n0, cplx)
        plan.lib.check(plan.lib.cwt_memcpy_d2h(plan.h, a.ctypes.data, Wa.ptr + i * n0 * es, a.nbytes))
        err = float(np.abs(a - ref[k]).max() / np.abs(ref[k]).max())
        assert err < TOL[prec], (i, classes[i], err)
    print("worst row error per class:", {k: f"{v:.1e}" for k, v in worst.items()})
    for b in (xd, xh, Wa, Wb):
        b.free()
    plan.close()


@pytest.mark.parametrize("config,tols,bar", [("c2", (1e-12, 1e-9, 1e-7), 1e-6), ("c3_dog", (1e-5, 3e-5), 1e-3)])
def test_tolerance_on_gpu(hip_library, monkeypatch, config, tols, bar):
    """The plan's accuracy target at the BASELINE size (N = 2^20): a sample of rows of every kernel class against the
    oracle stays inside the target (+ the arithmetic's own rounding), the default sits >= 100x inside north_star's bar,
    and a looser target never needs more two-pass rows."""
    import bench
    monkeypatch.delenv("CWT_TOLERANCE", raising=False)
    kind, param, prec, _ = bench.CONFIGS[config]
    N, rows = 1 << 20, 256
    m = orc.Mother(kind, int(param) if kind else param)
    sj = bench.scale_grid(N, 1.0, bench.flambda_of(kind, param), rows)
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    x = np.random.default_rng(1234).standard_normal(N).astype(real)
    xd, xh = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 2 * x.itemsize)
    Wd = _hip.DeviceBuffer(rows * N * 2 * x.itemsize)
    pick = np.arange(3, rows, 11)
    with np.errstate(all="ignore"):
        ref = orc.cwt_rows(x, 1.0, sj[pick], m)
    rounding = 1e-14 if prec == 64 else 8e-6
    two_pass = []
    for tol in (0.0,) + tuple(tols):
        plan = _hip.Plan(N, prec, max_rows=rows, options={"tolerance": tol})
        eff = plan.tolerance()
        assert eff == pytest.approx(tol if tol else (1e-16 if prec == 64 else 1e-8))
        xd.upload(plan, x)
        plan.transform(xd.ptr, N, kind, param, 1.0, sj, xh.ptr, Wd.ptr, N, N)
        classes = plan.row_classes()
        worst = 0.0
        for k, i in enumerate(pick):
            a = np.empty(N, cplx)
            plan.lib.check(plan.lib.cwt_memcpy_d2h(plan.h, a.ctypes.data, Wd.ptr + int(i) * N * 2 * x.itemsize, a.nbytes))
            worst = max(worst, float(np.abs(a - ref[k]).max() / np.abs(ref[k]).max()))
        assert worst < eff + rounding, (eff, worst)
        if tol == 0.0:
            assert worst < bar / 100, worst
        else:
            two_pass.append(sum(c.startswith("two_pass") for c in classes))
        plan.close()
    assert two_pass == sorted(two_pass, reverse=True), two_pass
    for b in (xd, xh, Wd):
        b.free()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_sample_on_gpu(hip_library, bad):
    """One NaN / inf sample at N = 2^18 (overlap-save rows on by default): the shim returns the reference's all-NaN W with
    every row kept (wavelet.py:91, :111-115); cwt_transform itself confines the damage of its overlap-save rows to the
    blocks around the sample (documented in cwt_hip.h) -- checked here so that the difference stays a known one."""
    n0 = (1 << 18) - 5
    x = np.random.default_rng(2).standard_normal(n0)
    x[100000] = bad
    W, sj, freqs, coi, fft, fftfreqs = pycwt_amd.cwt(x, 1.0, 0.5, -1, -1, "morlet")
    assert np.isnan(W).all() and not np.isfinite(fft).any()
    m = orc.Mother(orc.MORLET, 6)
    assert W.shape[0] == len(sj) == int(np.round(np.log2(n0 * 1.0 / (2 / m.flambda())) / 0.5)) + 1
    plan = _hip.Plan(1 << 18, 64, max_rows=len(sj))
    xd, xh, Wd = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(16 << 18), _hip.DeviceBuffer(len(sj) * n0 * 16)
    xd.upload(plan, x)
    plan.transform(xd.ptr, n0, orc.MORLET, 6, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
    classes = plan.row_classes()
    D = Wd.download(plan, (len(sj), n0), np.complex128)
    for i, c in enumerate(classes):
        if c.startswith("ols"):
            bad_cols = np.flatnonzero(~np.isfinite(D[i]))
            assert 0 < bad_cols.size <= 2 * 16384 and bad_cols.min() > 100000 - 16384 and bad_cols.max() < 100000 + 16384
        else:
            assert np.isnan(D[i]).all(), c
    assert any(c.startswith("ols") for c in classes)
    for b in (xd, xh, Wd):
        b.free()
    plan.close()


@pytest.mark.parametrize("name,prec", [("morlet", 64), ("paul", 32), ("dog", 32), ("morlet", 32)])
def test_round4_row_forms_against_the_forms_they_replace(hip_library, name, prec):
    """N = 2^20, every 3rd row of the bench grid: the polynomial rows (k_poly_*) and the rows clipped at Nyquist on the
    band-passed signal (k_aols_*) against the SAME rows through the kernels they replace (options poly = 0 / aols = 0:
    transform per residue, two-pass), row by row, and a sample of each against the oracle."""
    N = 1 << 20
    kind, param = MOTHERS[name]
    m = orc.Mother(kind, param)
    s0 = 2 / m.flambda()
    sj = (s0 * 2 ** (np.arange(256) * np.log2(N / s0) / 255))[::3]
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    x = np.random.default_rng(99).standard_normal(N - 1001).astype(real)
    n0 = x.size
    out = {}
    for tag, opts in (("new", None), ("old", {"poly": 0, "aols": 0})):
        plan = _hip.Plan(N, prec, max_rows=len(sj), options=opts)
        xd, xh = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 2 * x.itemsize)
        Wd = _hip.DeviceBuffer(len(sj) * n0 * 2 * x.itemsize)
        xd.upload(plan, x)
        plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        W = Wd.download(plan, (len(sj), n0), cplx)
        for b in (xd, xh, Wd):
            b.free()
        out[tag] = (W, plan.row_classes(), plan.last_split())
        plan.close()
    (Wn, cn, sn), (Wo, co, so) = out["new"], out["old"]
    assert sn["poly"] >= 30 and so["poly"] == 0 and so["aols"] == 0, (sn, so)
    if name != "dog":
        assert sn["aols"] >= 3 and sn["two_pass"] < so["two_pass"], (sn, so)
    finite = np.isfinite(Wo.view(real)).all(axis=1)
    assert finite.all() and np.isfinite(Wn.view(real)).all()
    per_row, _ = row_errors(Wn, Wo)
    assert per_row.max() < TOL[prec], (per_row.argmax(), cn[per_row.argmax()], co[per_row.argmax()], per_row.max())
    dropped = orc.dropped_rows(sj, 1.0, m)
    # (rows the reference turns into NaN included: the intended-value oracle has them)
    pick = (list(np.flatnonzero([c.startswith("aols") for c in cn])[:3]) +
            list(np.flatnonzero([c.startswith("poly") for c in cn])[::12]))
    if name == "paul":
        assert dropped[pick].any()
    with np.errstate(all="ignore"):
        ref = orc.cwt_rows(x, 1.0, sj[pick], m, N=N, intended=True)[:, :n0]
    per_row, _ = row_errors(Wn[pick], ref)
    assert per_row.max() < TOL[prec], (per_row, [cn[i] for i in pick])


def test_automatic_accuracy_of_the_shim_on_gpu(hip_library):
    """pycwt_amd's default mode: 1e-9 relative to every row's peak whatever the spectrum looks like: white
    noise runs at the fast target, a line 1e4 above the noise makes the call tighten its tolerance."""
    from pycwt_amd import wavelet
    N = 1 << 18
    noise = np.random.default_rng(12).standard_normal(N)
    line = noise + 1e4 * np.cos(2 * np.pi * 3 * np.arange(N) / N)
    m = orc.Mother(orc.MORLET, 6)
    keep = wavelet._tolerance
    try:
        pycwt_amd.set_tolerance("auto")
        used = {}
        for tag, x in (("noise", noise), ("line", line)):
            W, sj = pycwt_amd.cwt(x, 1.0, 0.5, -1, -1, "morlet")[:2]
            used[tag] = wavelet._plans[(N, 64, 0)].tolerance()
            per_row, _ = row_errors(W, orc.cwt_rows(x, 1.0, sj, m))
            assert per_row.max() < 1e-9, (tag, used[tag], per_row.max())
        assert used["noise"] == pytest.approx(1e-9) and used["line"] <= 1e-13, used
    finally:
        pycwt_amd.set_tolerance(keep)


def test_config4_full_batch_parseval_on_every_row(hip_library):
    """BASELINE config 4 at full size (VERDICT r03 "Next" 2e): ALL 131072 rows of the batch, not a sample, through the one
    identity that needs no inverse transform on the host -- Parseval per row,
        mean_n |W[b, j, n]|^2 = (1/N^2) sum_k |xhat_b[k]|^2 |F_j[k]|^2        (wavelet.py:102-106)
    with the left side from the device (cwt_time_mean_power over the device-resident W) and the right side from NumPy's FFT
    of the signals and the filter bank.  A wrong row of any kernel class, signal or scale shows up here."""
    nb, N, rows = 1024, 1 << 16, 128
    m = orc.Mother(orc.MORLET, 6)
    s0 = 2 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))
    X = np.random.default_rng(4321).standard_normal((nb, N))
    plan = _hip.Plan(N, 64, max_rows=nb * rows)
    xd, xh = _hip.DeviceBuffer(X.nbytes), _hip.DeviceBuffer(nb * N * 16)
    Wd, pw = _hip.DeviceBuffer(nb * rows * N * 16), _hip.DeviceBuffer(nb * rows * 8)
    xd.upload(plan, X)
    plan.transform_batch(xd.ptr, nb, N, N, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
    plan.time_mean_power(Wd.ptr, N, N, nb * rows, pw.ptr)
    got = pw.download(plan, (nb, rows), np.float64)
    classes = plan.row_classes()
    for b in (xd, xh, Wd, pw):
        b.free()
    plan.close()
    power = np.abs(np.fft.fft(X, axis=1)) ** 2                                   # (nb, N)
    bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m)                  # (rows, N), wavelet.py:102-104
    want = power @ (np.abs(bank) ** 2).T / float(N) ** 2
    rel = np.abs(got - want) / want
    b, j = np.unravel_index(rel.argmax(), rel.shape)
    print(f"config 4, Parseval on all {nb * rows} rows: worst relative deviation {rel.max():.2e} at signal {b}, scale {j} "
          f"({classes[j]})")
    assert rel.max() < 1e-10, (b, j, classes[j], rel.max())


@pytest.mark.parametrize("prec,tol", [(64, 2e-14), (32, 2e-5)])
@pytest.mark.parametrize("name", ["morlet", "paul", "dog"])
@pytest.mark.parametrize("n0", [16, 504, 1000, 4096])
def test_short_calls_on_gpu(hip_library, prec, tol, name, n0):
    """Transforms that fit one workgroup per row: kernels that read the signal and write W through page-locked host memory
    (cwt_execute_host; the default), against the staged form (copy operations) and the oracle."""
    kind, param = MOTHERS[name]
    m = orc.Mother(kind, param)
    N = 1 << int(np.ceil(np.log2(n0)))
    x = np.random.default_rng(n0).standard_normal(n0)
    sj = grid(n0, 0.25, m, 41)
    out = {}
    for label, opts in (("fused", {}), ("staged", {"host_direct": 0})):
        plan = _hip.Plan(N, prec, max_rows=len(sj), lib=hip_library, options=opts)
        out[label] = plan.execute_host(x, kind, param, 0.25, sj)
        assert set(plan.row_classes()) == {"single_wg"}
        plan.close()
    np.testing.assert_array_equal(out["fused"][0], out["staged"][0])          # the same kernels on the same values
    np.testing.assert_array_equal(out["fused"][1], out["staged"][1])
    per_row, l2 = row_errors(out["fused"][0], orc.cwt_rows(x, 0.25, sj, m, N=N)[:, :n0])
    assert per_row.max() < tol and l2 < tol, (per_row.max(), l2)


def test_shim_results_live_in_their_own_page_locked_buffers(hip_library):
    g = load_golden("nino3_simple")
    outs = [pycwt_amd.cwt(g["x"] * k, 0.25, 1 / 12, 0.5, 84, "morlet") for k in (1.0, 2.0, 3.0)]
    assert len({o[0].ctypes.data for o in outs}) == 3
    for k, o in zip((1.0, 2.0, 3.0), outs):
        per_row, _ = row_errors(o[0], k * g["W"])
        assert per_row.max() < 1e-12
    check_tuple(outs[0], g, 1e-12)
    pool = hip_library.pinned
    assert pool.total > 0
    before = sum(len(v) for v in pool.free.values())
    del outs, o
    import gc
    gc.collect()
    assert sum(len(v) for v in pool.free.values()) >= before + 3


def test_both_schedules_and_every_stream_placement_keep_every_bit(hip_library):
    """cwt_transform (the call that has the signal: overlap-save, band-passed and polynomial rows on up to five streams):
    where a launch is queued must not change a bit of W -- the serial schedule (the fp64 default) and the round-5 schedule
    (serial_rows = 0), the block spectra early or late, the polynomial rows beside the others or behind them, everything on
    the plan's own stream."""
    N = 1 << 20
    x = np.random.default_rng(78).standard_normal(N)
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, 1.0, m, 256)[:128:2]                     # 64 rows: overlap-save on both tile sizes, band-passed, polynomial
    base = None
    for opts in (None, {"ols_early": 0}, {"overlap_narrow": 0}, {"overlap_narrow": 0, "ols_early": 0, "ols_side": 0},
                 {"serial_rows": 0}):      # (the default is the serial schedule 2)
        plan = _hip.Plan(N, 64, max_rows=64, options=dict(opts or {}, tolerance=1e-9))
        xd, xh, Wd = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 16), _hip.DeviceBuffer(len(sj) * N * 16)
        xd.upload(plan, x)
        for _ in range(3):
            plan.transform(xd.ptr, N, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
        W = Wd.download(plan, (len(sj), N), np.complex128)
        split = plan.last_split()
        for b in (xd, xh, Wd):
            b.free()
        plan.close()
        if base is None:
            base = W
            assert split["ols"] >= 8 and split["aols"] >= 3 and split["poly"] >= 8, split
            idx = [0, 20, 40, 63]
            per_row, _ = row_errors(W[idx], orc.cwt_rows(x, 1.0, sj[idx], m))
            assert per_row.max() < 1e-8
        else:
            assert np.array_equal(W, base), opts


def test_replaced_side_streams_keep_every_bit(hip_library):
    """The plan checks that its four streams sit on four hardware queues and replaces side streams that share one (streams
    made earlier in the process shift the runtime's assignment).  Streams are only WHERE work is queued: with one, two and
    three older streams in the way -- every assignment of the runtime's round -- W keeps the bits of a plan that takes its
    streams as they come."""
    import torch
    N = 1 << 20
    x = np.random.default_rng(79).standard_normal(N)
    sj = grid(N, 1.0, orc.Mother(orc.MORLET, 6), 256)[:128:2]
    older, base = [], None
    for probe in (0, 1, 1, 1):
        plan = _hip.Plan(N, 64, max_rows=64, options={"tolerance": 1e-9, "queue_probe": probe})
        xd, xh, Wd = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 16), _hip.DeviceBuffer(len(sj) * N * 16)
        xd.upload(plan, x)
        for _ in range(3):
            plan.transform(xd.ptr, N, orc.MORLET, 6.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
        W = Wd.download(plan, (len(sj), N), np.complex128)
        for b in (xd, xh, Wd):
            b.free()
        plan.close()
        if base is None:
            base = W
        else:
            assert np.array_equal(W, base), len(older)
        st = torch.cuda.Stream()                          # one more stream in the way of the next plan's
        with torch.cuda.stream(st):
            torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        older.append(st)


def test_polynomial_rows_in_chunks_at_full_size(hip_library):
    """fp64 Paul at the bench target: 150 MB of coefficient planes, so the polynomial rows go through in two chunks (planes
    computed, consumed, next chunk).  Same bits as all rows at once; a few rows against the forms the polynomial one replaced
    (the reference has no values for these scales: they are the rows its Paul filter turns into NaN, wavelet.py:111-115)."""
    N = 1 << 20
    m = orc.Mother(orc.PAUL, 4)
    s0 = 2 / m.flambda()
    sj_all = s0 * 2 ** (np.arange(256) * np.log2(N / s0) / 255)
    x = np.random.default_rng(1234).standard_normal(N)
    out = {}
    for mb in (96, 0, 24):
        plan = _hip.Plan(N, 64, max_rows=256, options={"tolerance": 1e-9, "poly_chunk_mb": mb})
        labels = plan.classify(orc.PAUL, 4.0, 1.0, sj_all, N)
        idx = [j for j, l in enumerate(labels) if l.startswith("poly/")]
        assert len(idx) >= 120
        sj = sj_all[idx]
        xd, xh, Wd = _hip.DeviceBuffer(x.nbytes), _hip.DeviceBuffer(N * 16), _hip.DeviceBuffer(len(sj) * N * 16)
        xd.upload(plan, x)
        plan.transform(xd.ptr, N, orc.PAUL, 4.0, 1.0, sj, xh.ptr, Wd.ptr, N, N)
        assert plan.last_split()["poly"] == len(sj)
        heavy = [k for k, j in enumerate(idx) if "K16384" in labels[j] or "K8192" in labels[j]]
        out[mb] = np.concatenate([_download_rows(plan, Wd, k, 1, N, np.complex128) for k in heavy[::3]])
        if mb == 96:
            pick = heavy[::3][:4]
            old = _hip.Plan(N, 64, max_rows=8, options={"tolerance": 1e-9, "poly": 0})
            Wo = _hip.DeviceBuffer(len(pick) * N * 16)
            old.transform(xd.ptr, N, orc.PAUL, 4.0, 1.0, sj[pick], xh.ptr, Wo.ptr, N, N)
            assert old.last_split()["poly"] == 0
            ref = Wo.download(old, (len(pick), N), np.complex128)
            Wo.free()
            old.close()
            want = orc.cwt_rows(x, 1.0, sj[pick], m, intended=True)     # these scales are rows the reference drops
            assert (sj[pick] * np.pi > 709.7827).all()            # (SURVEY 8a quirk iii: exp(-f) overflows at the Nyquist bin)
            for i, k in enumerate(pick):
                got = _download_rows(plan, Wd, k, 1, N, np.complex128)[0]
                assert np.isfinite(got.view(np.float64)).all()
                assert np.abs(got - ref[i]).max() < 1e-8 * np.abs(ref[i]).max()
                assert np.abs(got - want[i]).max() < 1e-8 * np.abs(want[i]).max()
        for b in (xd, xh, Wd):
            b.free()
        plan.close()
    assert np.array_equal(out[96], out[0]) and np.array_equal(out[24], out[0])


def test_device_resident_coherence_and_device_surrogates_on_gpu(hip_library, tmp_path, monkeypatch):
    """SURVEY 8f-2 / VERDICT r04 next #7 on the GPU: `wct_device` / `xwt_device` hold the bits `wct(sig=False)` / `xwt` return;
    the Monte-Carlo levels with surrogates made on the device (Philox, `cwt_random_normal`, `cwt_ar1_filter`) agree with the
    NumPy-surrogate path within the Monte-Carlo error (two NumPy runs with different seeds are the yardstick)."""
    from pycwt_amd import wavelet
    monkeypatch.setattr(wavelet, "get_cache_dir", lambda: str(tmp_path) + "/")
    n = 1 << 18
    rng = np.random.default_rng(9)
    e = rng.standard_normal(n)
    y1 = e + np.sin(2 * np.pi * np.arange(n) / 300.0)
    y2 = 0.5 * np.roll(e, 2) + rng.standard_normal(n)
    WCT, aWCT, coi, freq, _ = pycwt_amd.wct(y1, y2, 1.0, 0.5, sig=False)
    with pycwt_amd.wct_device(y1, y2, 1.0, 0.5) as D:
        assert np.array_equal(D.wct(), WCT) and np.array_equal(D.angle(), aWCT)
    W12 = pycwt_amd.xwt(y1, y2, 1.0, 0.5)[0]
    T, _ = pycwt_amd.xwt_device(y1, y2, 1.0, 0.5)
    assert np.array_equal(T.W(), W12)
    T.close()
    for surrogates, al in (("reference", (0.3, 0.5)), ("ar1", (0.6, 0.8))):
        kw = dict(dt=1.0, dj=0.5, s0=2.0, J=8, mc_count=300, progress=False, wavelet="morlet", surrogates=surrogates, cache=False)
        np.random.seed(1)
        host_a = pycwt_amd.wct_significance(*al, **kw)
        np.random.seed(2)
        host_b = pycwt_amd.wct_significance(*al, **kw)
        dev_a = pycwt_amd.wct_significance(*al, rng="device", seed=11, **kw)
        dev_b = pycwt_amd.wct_significance(*al, rng="device", seed=12, **kw)
        ok = np.isfinite(host_a)
        np.testing.assert_array_equal(np.isnan(dev_a), np.isnan(host_a))
        yard = max(np.abs(host_a[ok] - host_b[ok]).max(), np.abs(dev_a[ok] - dev_b[ok]).max(), 0.01)
        assert np.abs(dev_a[ok] - host_a[ok]).max() <= 2.5 * yard, (surrogates, dev_a, host_a, yard)
        np.testing.assert_array_equal(pycwt_amd.wct_significance(*al, rng="device", seed=11, **kw), dev_a)
