"""The cases of tests/shrink_common.py on the GPU: cwt_row_order_statistics, cwt_icwt_shrink and the shim around them, in both
precisions, at the shapes of tests/test_shrink_emulated.py plus rows of 2^17 + 3 columns (a row spans workgroups: the global
histogram and the compaction counter take adds from many of them)."""
import pytest

import pycwt_amd
import shrink_common as sc
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, hip_library):
    with sc.Dev(hip_library, sc.NFFT, request.param, max_rows=sc.ROWS_W) as d:
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


@pytest.mark.parametrize("nrows,ncols,first_kind", sc.SELECT_CASES + sc.SELECT_CASES_GPU)
def test_selection_of_reals_is_exact(dev, nrows, ncols, first_kind):
    sc.check_select_real(dev, nrows, ncols, first_kind)


@pytest.mark.parametrize("nrows,ncols,first_kind", [c for c in sc.SELECT_CASES + sc.SELECT_CASES_GPU if c[0] == 3])
def test_selection_of_complex_adversarial_rows(dev, nrows, ncols, first_kind):
    sc.check_select_complex_rows(dev, nrows, ncols, first_kind)


def test_selection_on_a_real_transform(dev):
    sc.check_select_complex_w(dev)


def test_refusals_touch_nothing(dev):
    codes, untouched = sc.refusals(dev)
    assert all(rc == sc.EINVAL for _, rc in codes), [c for c in codes if c[1] != sc.EINVAL]
    assert len(codes) >= 24 and untouched


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("nrows,ncols,pattern", sc.CASES)
def test_shrink_inverse_against_long_double(dev, nrows, ncols, pattern, mode):
    sc.check_shrink(dev, nrows, ncols, pattern, mode)


def test_special_entries(dev):
    sc.check_special_entries(dev)


@pytest.mark.parametrize("ncols", sc.SHRINK_NCOLS)
@pytest.mark.parametrize("nrows", sc.SHRINK_ROWS)
def test_zero_thresholds_in_hard_mode_are_icwt_reduce_bit_for_bit(dev, nrows, ncols):
    sc.check_bit_identity(dev, nrows, ncols)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_scratch_reuse_keeps_every_bit(hip_library, prec):
    sc.check_scratch_reuse(hip_library, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_order_statistics_between_two_transforms_on_a_live_plan(hip_library, prec):
    sc.check_live_plan_sequence(hip_library, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(sc.E2E_MOTHERS))
def test_denoise_against_the_oracle_pipeline(hip_library, shim, name, prec):
    assert TOL == sc.TOL
    sc.check_oracle_parity(name, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_denoise_with_a_noise_window(hip_library, shim, prec):
    sc.check_oracle_parity("morlet", prec, columns=(0, 1000))


@pytest.mark.parametrize("prec", sc.PRECS)
def test_thresholds_quantiles_and_refusals_of_the_shim(hip_library, shim, prec):
    sc.check_denoise_surface(prec)


def test_hard_universal_threshold_halves_the_noise(hip_library, shim):
    sc.check_functional()
