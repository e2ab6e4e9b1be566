"""test_switch_scales_emulated.py's cases on the MI355X, through the same builders and within the same bounds: the values at
every switch pair (A) at N = 2^15 with FORMS_OPTS and at 2^18 with the default options, the power and weighted outputs (C), the
adjoint (D) and ncols != n0 (E) at 2^15 -- and A at N = 2^20 with the default options and n0 = 2^20 - 77, where the classifier
runs as bench.py runs it: fp64 Morlet(6) and fp32 DOG(2) on white noise, at round-off and at the bench target, at most 64 pair
rows per call (pairs of families already represented are dropped, never a whole family: switch_common.thin), so that W is 1 GiB
at most and the oracle of the rows a few seconds of host time.

The switch pairs are searched on the plan of the test, i.e. with the classifier as the product library was built: the host
compiler may place a switch an ulp apart from the emulation's, the families (switch_common.FAMILIES) are the same."""
import pytest

import switch_common as sc
import test_switch_scales_emulated as emu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sc.value_cases(15), ids=sc.case_id)
def test_values_at_every_switch_pair(hip_library, case):
    emu.check_values(hip_library, *case)


@pytest.mark.parametrize("case", sc.value_cases(18), ids=sc.case_id)
def test_values_at_every_switch_pair_of_the_production_gates(hip_library, case):
    emu.check_values(hip_library, *case)


@pytest.mark.parametrize("case", sc.flagship_cases(), ids=sc.case_id)
def test_values_at_the_switch_pairs_of_the_flagship_length(hip_library, case):
    emu.check_values(hip_library, *case, most=sc.FLAGSHIP_ROWS // 2)


@pytest.mark.parametrize("case", emu.output_cases(), ids=lambda c: sc.case_id(c + ("white",)))
def test_power_and_weighted_outputs_at_the_pairs(hip_library, case):
    emu.check_power_and_weighted(hip_library, *case)


@pytest.mark.parametrize("prec,kind,param,adjoint_poly", emu.adjoint_cases(), ids=lambda v: None if v is None else str(v))
def test_adjoint_at_the_pairs(hip_library, prec, kind, param, adjoint_poly):
    emu.check_adjoint(hip_library, prec, kind, param, adjoint_poly)


@pytest.mark.parametrize("case", emu.shape_cases(), ids=emu.shape_id)
def test_ncols_other_than_n0_and_a_padded_leading_dimension(hip_library, case):
    emu.check_shape(hip_library, *case)


@pytest.mark.parametrize("case", emu.POWER_SHAPE_CASES, ids=emu.shape_id)
def test_power_with_ncols_other_than_n0(hip_library, case):
    emu.check_shape_power(hip_library, *case)
