"""Wavelet shrinkage on the CPU emulation of the HIP runtime: cwt_row_order_statistics, cwt_icwt_shrink and the shim around them
(row_quantiles, noise_levels, icwt_shrink, denoise).  The cases, references and bounds are in tests/shrink_common.py; the same
cases run on the device in tests/test_shrink_gpu.py."""
import os

import pytest

import shrink_common as sc
from conftest import ROOT


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, emu_library):
    with sc.Dev(emu_library, sc.NFFT, request.param, max_rows=sc.ROWS_W) as d:
        yield d


# ---- 1. cwt_row_order_statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows,ncols,first_kind", sc.SELECT_CASES)
def test_selection_of_reals_is_exact(dev, nrows, ncols, first_kind):
    sc.check_select_real(dev, nrows, ncols, first_kind)


@pytest.mark.parametrize("nrows,ncols,first_kind", [c for c in sc.SELECT_CASES if c[0] == 3])
def test_selection_of_complex_adversarial_rows(dev, nrows, ncols, first_kind):
    sc.check_select_complex_rows(dev, nrows, ncols, first_kind)


def test_selection_on_a_real_transform(dev):
    sc.check_select_complex_w(dev)


def test_refusals_touch_nothing(dev):
    codes, untouched = sc.refusals(dev)
    assert all(rc == sc.EINVAL for _, rc in codes), [c for c in codes if c[1] != sc.EINVAL]
    assert len(codes) >= 24 and untouched


# ---- 2. cwt_icwt_shrink ------------------------------------------------------------------------------------------------------------
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
def test_scratch_reuse_keeps_every_bit(emu_library, prec):
    sc.check_scratch_reuse(emu_library, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_order_statistics_between_two_transforms_on_a_live_plan(emu_library, prec):
    sc.check_live_plan_sequence(emu_library, prec)


# ---- 3. the shim -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(sc.E2E_MOTHERS))
def test_denoise_against_the_oracle_pipeline(emulated, name, prec):
    sc.check_oracle_parity(name, prec)


@pytest.mark.parametrize("prec", sc.PRECS)
def test_denoise_with_a_noise_window(emulated, prec):
    sc.check_oracle_parity("morlet", prec, columns=(0, 1000))


@pytest.mark.parametrize("prec", sc.PRECS)
def test_thresholds_quantiles_and_refusals_of_the_shim(emulated, prec):
    sc.check_denoise_surface(prec)


def test_hard_universal_threshold_halves_the_noise(emulated):
    sc.check_functional()


# ---- 4. documents ------------------------------------------------------------------------------------------------------------------
def test_header_and_accuracy_record():
    text = open(os.path.join(ROOT, "include", "cwt_hip.h")).read()
    assert "int cwt_row_order_statistics(" in text and "int cwt_icwt_shrink(" in text
    assert set(sc.MEASURED) == set(sc.PRECS), sc.ACCURACY_FILE
