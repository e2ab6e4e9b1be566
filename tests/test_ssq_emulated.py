"""The synchrosqueezed transform on the CPU emulation of the kernels (tests/emu): cwt_spectrum_derivative, cwt_ssq_reassign and the
shim around them (ssq_cwt, ssq_cwt_device, issq_cwt) against the definition restated in tests/ssq_common.py.  The same case
functions run on the GPU in tests/test_ssq_gpu.py."""
import numpy as np
import pytest

import pycwt_amd
import ssq_common as sc
from pycwt_amd import wavelet
from test_gpu_parity import TOL


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, emu_library):
    with sc.Dev(emu_library, 16, request.param, max_rows=64) as d:
        yield d


# ---- 1. cwt_ssq_reassign on synthetic matrices -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", sc.NFS)
@pytest.mark.parametrize("ncols", sc.NCOLS)
@pytest.mark.parametrize("rows", sc.ROWS)
def test_reassign_synthetic(dev, rows, ncols, nf):
    sc.check_synthetic(dev, rows, ncols, nf)


def test_row_chunks_give_the_same_bits_and_accumulate_adds(dev):
    sc.check_chunks_and_accumulate(dev)


def test_refusals_launch_nothing_and_touch_nothing(dev, emu_library):
    dev.plan.sync()
    emu_library.dll.hipemu_clear_launched()
    codes, untouched = sc.refusals(dev)
    assert all(rc == sc.EINVAL for _, rc in codes), [c for c in codes if c[1] != sc.EINVAL]
    assert len(codes) >= 28 and untouched
    assert not sc.launch_log(emu_library), sc.launch_log(emu_library)


# ---- 2. cwt_spectrum_derivative ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("N", [16, 1 << 15])
def test_spectrum_derivative(emu_library, N, prec):
    with sc.Dev(emu_library, N, prec, max_rows=8) as d:
        sc.check_spectrum_derivative(d, N)


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("n0", [1000, 1 << 15])
@pytest.mark.parametrize("mother", list(sc.MOTHERS))
def test_derivative_rows_against_the_oracle(emu_library, mother, n0, prec):
    N = 1 << int(np.ceil(np.log2(n0)))
    with sc.Dev(emu_library, N, prec, max_rows=64) as d:
        sc.check_derivative_rows(d, mother, n0, 24, TOL[prec])


# ---- 3. a tone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("mother", list(sc.MOTHERS))
@pytest.mark.parametrize("N", [1024, 1 << 15])
def test_tone_lands_in_one_bin(emulated, N, mother, prec):
    sc.check_tone(N, mother, prec)


# ---- 4. noise plus a chirp --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("n0,dj,seed", [(1000, 1 / 12, 11), ((1 << 15) + 3, 1 / 4, 12)])
def test_noise_plus_chirp(emulated, n0, dj, seed, prec):
    out = sc.check_noise_chirp(n0, prec, dj, seed)
    print(n0, prec, out)


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_surface(emulated):
    x, _ = sc.chirp_in_noise(300, 1)
    Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt(x, 0.5)
    W, sj2, freqs2, coi2 = pycwt_amd.cwt(x, 0.5)[:4]
    nf = int(np.round(np.log2(freqs.max() / freqs.min()) * 12)) + 1
    assert Tx.shape == (nf, 300) and Tx.dtype == np.complex128 and fs.shape == (nf,) and np.all(np.diff(fs) > 0)
    assert np.array_equal(fs, freqs.min() * 2.0 ** ((1 / 12) * np.arange(nf)))
    assert np.array_equal(sj, sj2) and np.array_equal(freqs, freqs2) and np.array_equal(coi, coi2)
    H = pycwt_amd.ssq_cwt_device(x, 0.5)
    D = pycwt_amd.cwt_device(x, 0.5)
    try:
        assert isinstance(H, pycwt_amd.DeviceSynchrosqueezed)
        assert np.array_equal(H.T(), Tx) and np.array_equal(H.ssq_freqs, fs)
        assert np.array_equal(H.W().view(np.float64), D.W().view(np.float64))             # the bits of cwt_device
        assert H.W().shape == W.shape and H.dW().shape == W.shape
        back = H.issq(1 / 12)
        assert back.shape == (300,) and np.array_equal(back, pycwt_amd.issq_cwt(Tx, 0.5, 1 / 12))
    finally:
        H.close()
        H.close()                                                                        # idempotent
        D.close()
    assert H._buf is None and H._Wbuf is None and H._spectrum is None
    # single precision computes in complex64 and widens; rows chunked through the scratch pool: the same T
    T32 = pycwt_amd.ssq_cwt(x, 0.5, precision=32)[0]
    assert T32.dtype == np.complex128 and np.array_equal(T32, T32.astype(np.complex64))
    keep = wavelet.SSQ_CHUNK_ROWS
    try:
        wavelet.SSQ_CHUNK_ROWS = 7
        assert np.array_equal(pycwt_amd.ssq_cwt(x, 0.5)[0], Tx)
    finally:
        wavelet.SSQ_CHUNK_ROWS = keep
    # an explicit grid, and a caller's freqs= with one
    Tg, fg = pycwt_amd.ssq_cwt(x, 0.5, ssq_freqs=(0.05, 1 / 6, 9))[:2]
    assert Tg.shape == (9, 300) and np.array_equal(fg, 0.05 * 2.0 ** ((1 / 6) * np.arange(9)))
    Tf = pycwt_amd.ssq_cwt(x, 0.5, freqs=freqs[::2], ssq_freqs=(0.05, 1 / 6, 9))
    assert Tf[0].shape == (9, 300) and Tf[2].shape == freqs[::2].shape


def test_paul_drops_the_rows_cwt_drops(emulated):
    x, _ = sc.chirp_in_noise(256, 2)
    full = pycwt_amd.wavelet._scale_grid(pycwt_amd.Paul(4), 256, 1.0, 1 / 4, -1, -1, None)[0]
    Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt(x, 1.0, 1 / 4, wavelet="paul")
    sj_cwt = pycwt_amd.cwt(x, 1.0, 1 / 4, wavelet="paul")[1]
    assert np.array_equal(sj, sj_cwt) and sj.size < full.size and np.isfinite(Tx).all()
    assert fs[0] == freqs.min() and fs.size == int(np.round(np.log2(freqs.max() / freqs.min()) * 4)) + 1


def test_value_errors(emulated):
    x, _ = sc.chirp_in_noise(128, 3)

    class Duck:
        def psi_ft(self, f):
            return pycwt_amd.Morlet(6).psi_ft(f)

        def flambda(self):
            return pycwt_amd.Morlet(6).flambda()

        def coi(self):
            return pycwt_amd.Morlet(6).coi()
    for kw in (dict(wavelet="dog"), dict(wavelet="mexicanhat"), dict(wavelet=pycwt_amd.DOG(3)), dict(wavelet=Duck()), dict(pad=False),
               dict(freqs=np.array([0.1, 0.2])), dict(ssq_freqs=(0.0, 1 / 12, 5)), dict(ssq_freqs=(0.1, 1 / 12)), dict(gamma=-1.0),
               dict(gamma=np.nan)):
        for fn in (pycwt_amd.ssq_cwt, pycwt_amd.ssq_cwt_device):
            with pytest.raises(ValueError):
                fn(x, 1.0, **kw)
    for kw in (dict(hop=2), dict(pool=2)):
        with pytest.raises(TypeError):
            pycwt_amd.ssq_cwt(x, 1.0, **kw)
    with pytest.raises(ValueError):
        pycwt_amd.issq_cwt(np.zeros((4, 8), dtype=complex), 1.0, band=(0.1, 0.2))             # a band without the bins' frequencies


def test_nan_signal_gives_nan_everywhere(emulated):
    x, _ = sc.chirp_in_noise(128, 4)
    x[17] = np.nan
    Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt(x, 1.0)
    W, sj2 = pycwt_amd.cwt(x, 1.0)[:2]
    assert np.isnan(Tx.real).all() and np.isnan(Tx.imag).all() and np.isnan(W).all() and np.array_equal(sj, sj2)
    assert Tx.shape == (fs.size, 128)
