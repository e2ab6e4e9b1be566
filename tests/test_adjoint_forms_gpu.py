"""test_adjoint_forms_emulated.py's cases on the MI355X -- every row alone (A), single tones (B), polynomial chunks (C), row order
(D) and the cached tables of a live plan (E), at the same small shapes and bounds, through the same case builders -- and the two
shapes only a GPU can afford: N = 2^22 and 2^23 with K' held at 256, where k_poly_moments' LDS tree is the full 256 lanes wide
(logR = 14) and a thread sums L = 128 samples instead of 64 (logR = 15).

Bounds of the long series: test_adjoint_emulated.BOUND per row, unchanged.  The N-point transforms of reference and kernel lose
~eps log2 N: 2.6e-15 in fp64 and 1.4e-6 in complex64 at N = 2^23, inside 1e-12 / 1e-5 (the float64 reference itself against the
longdouble closed form: test_adjoint_forms_emulated.test_reference_own_error)."""
import numpy as np
import pytest

from oracle import cwt_oracle as orc
import test_adjoint_forms_emulated as forms
from test_adjoint_emulated import BOUND

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,param,prec,n0_off,target", [(orc.MORLET, 6, 64, 0, "roundoff"), (orc.MORLET, 6, 64, 77, "bench"),
                                                            (orc.DOG, 3, 32, 0, "roundoff"), (orc.DOG, 3, 32, 77, "roundoff"),
                                                            (orc.DOG, 3, 32, 0, "bench")])
def test_every_row_alone(hip_library, kind, param, prec, n0_off, target):
    forms.test_every_row_alone(hip_library, kind, param, prec, n0_off, target)


@pytest.mark.parametrize("kind,param,prec,target", [(orc.MORLET, 6, 64, "bench"), (orc.DOG, 3, 32, "bench"),
                                                    (orc.DOG, 2, 64, "bench")])
def test_single_tones_against_the_closed_form(hip_library, kind, param, prec, target):
    forms.test_single_tones_against_the_closed_form(hip_library, kind, param, prec, target)


def test_paul_single_tones_through_the_polynomial_form(hip_library):
    forms.test_paul_single_tones_through_the_polynomial_form(hip_library, 64, "bench")


def test_paul_rows_alone_through_the_polynomial_form(hip_library):
    forms.test_paul_rows_alone_through_the_polynomial_form(hip_library, 64, "bench")


@pytest.mark.parametrize("kind,param,prec", [(orc.MORLET, 6, 64), (orc.DOG, 2, 32), (orc.MORLET, 6, 32)])
def test_polynomial_rows_in_three_or_more_chunks(hip_library, kind, param, prec):
    forms.test_polynomial_rows_in_three_or_more_chunks(hip_library, kind, param, prec)


@pytest.mark.parametrize("kind,param,prec,target", [(orc.MORLET, 6, 64, "bench"), (orc.DOG, 3, 32, "roundoff")])
def test_unsorted_repeated_and_subset_scales(hip_library, kind, param, prec, target):
    forms.test_unsorted_repeated_and_subset_scales(hip_library, kind, param, prec, target)


def test_more_row_tables_than_slots(hip_library):
    forms.test_more_row_tables_than_slots(hip_library)


def test_tolerance_changed_between_calls(hip_library):
    forms.test_tolerance_changed_between_calls(hip_library)


def test_adjoint_poly_toggled_on_a_live_plan(hip_library):
    forms.test_adjoint_poly_toggled_on_a_live_plan(hip_library)


def test_forward_with_a_padded_leading_dimension_then_the_adjoint(hip_library):
    forms.test_forward_with_a_padded_leading_dimension_then_the_adjoint(hip_library)


def test_padded_rows_and_padded_batch_entries_of_the_input(hip_library):
    forms.test_padded_rows_and_padded_batch_entries_of_the_input(hip_library)


def test_row_counts_the_plan_cannot_hold_are_refused_before_any_launch(hip_library):
    forms.test_row_counts_the_plan_cannot_hold_are_refused_before_any_launch(hip_library)


@pytest.mark.parametrize("logn", [22, 23])
@pytest.mark.parametrize("kind,param,prec", [(orc.MORLET, 6, 64), (orc.DOG, 2, 32)])
def test_long_series_full_width_tree_and_long_thread_sums(hip_library, kind, param, prec, logn):
    """Three rows of the largest scales, each alone, polynomial with K' = 256 (asserted): per row against the NumPy adjoint in
    both metrics, through the transpose of the polynomial form and through the general path."""
    (poly, general), classes = forms.run_long(hip_library, logn, kind, param, prec)
    print(logn, classes, "adjoint_poly = 1:", poly, "adjoint_poly = 0:", general)
    assert all(c.startswith("poly/K256/") for c in classes), classes
    for errs in (poly, general):
        assert max(errs[0].max(), errs[1].max()) <= BOUND[prec], (classes, errs)
