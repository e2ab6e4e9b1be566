"""The case functions of tests/ssq_common.py on the GPU: cwt_spectrum_derivative, cwt_ssq_reassign and the shim around them, in
both precisions, at the shapes of tests/test_ssq_emulated.py plus the ones only a GPU makes cheap (64 x 65539 synthetic entries:
more than 512 workgroups, a last one of 3 lanes; noise plus a chirp at 2^18 samples)."""
import numpy as np
import pytest

import pycwt_amd
import ssq_common as sc
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, hip_library):
    with sc.Dev(hip_library, 16, request.param, max_rows=64) as d:
        yield d


@pytest.fixture()
def shim():
    """the shim's plans of this test, closed when it ends"""
    from pycwt_amd import wavelet
    yield
    for p in wavelet._plans.values():
        p.close()
    wavelet._plans.clear()
    pycwt_amd.release_scratch()


@pytest.mark.parametrize("nf", sc.NFS)
@pytest.mark.parametrize("rows", sc.ROWS)
def test_reassign_synthetic(dev, rows, nf):
    for ncols in sc.NCOLS:
        sc.check_synthetic(dev, rows, ncols, nf)


def test_reassign_synthetic_many_workgroups(dev):
    sc.check_synthetic(dev, 64, 65539, 40)


def test_row_chunks_give_the_same_bits_and_accumulate_adds(dev):
    sc.check_chunks_and_accumulate(dev)


def test_refusals_touch_nothing(dev):
    codes, untouched = sc.refusals(dev)
    assert all(rc == sc.EINVAL for _, rc in codes), [c for c in codes if c[1] != sc.EINVAL]
    assert len(codes) >= 28 and untouched


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("N", [16, 1 << 15])
def test_spectrum_derivative(hip_library, N, prec):
    with sc.Dev(hip_library, N, prec, max_rows=8) as d:
        sc.check_spectrum_derivative(d, N)


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("n0", [1000, 1 << 15])
@pytest.mark.parametrize("mother", list(sc.MOTHERS))
def test_derivative_rows_against_the_oracle(hip_library, mother, n0, prec):
    N = 1 << int(np.ceil(np.log2(n0)))
    with sc.Dev(hip_library, N, prec, max_rows=64) as d:
        sc.check_derivative_rows(d, mother, n0, 24, TOL[prec])


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("mother", list(sc.MOTHERS))
@pytest.mark.parametrize("N", [1024, 1 << 15])
def test_tone_lands_in_one_bin(hip_library, shim, N, mother, prec):
    sc.check_tone(N, mother, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_noise_plus_chirp(hip_library, shim, prec):
    out = sc.check_noise_chirp(1 << 18, prec, 1 / 4, 13)
    print(prec, out)


def test_python_surface(hip_library, shim):
    x, _ = sc.chirp_in_noise(300, 1)
    Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt(x, 0.5)
    assert Tx.shape == (fs.size, 300) and Tx.dtype == np.complex128
    H, D = pycwt_amd.ssq_cwt_device(x, 0.5), pycwt_amd.cwt_device(x, 0.5)
    try:
        assert np.array_equal(H.T(), Tx) and np.array_equal(H.W().view(np.float64), D.W().view(np.float64))
        assert np.array_equal(H.issq(1 / 12), pycwt_amd.issq_cwt(Tx, 0.5, 1 / 12))
    finally:
        H.close()
        H.close()
        D.close()
    x[5] = np.inf
    assert np.isnan(pycwt_amd.ssq_cwt(x, 0.5)[0]).all()
