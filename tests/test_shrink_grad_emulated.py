"""The gradient of wavelet shrinkage on the CPU emulation of the HIP runtime: cwt_icwt_shrink_adjoint and the torch entry points
icwt_torch, icwt_shrink_torch and denoise_torch.  The cases, references and bounds are in tests/shrink_grad_common.py; the same
cases run on the device in tests/test_shrink_grad_gpu.py."""
import os

import pytest

import shrink_grad_common as gc
from conftest import ROOT

torch = pytest.importorskip("torch")
CPU = torch.device("cpu")


@pytest.fixture(scope="module", params=gc.PRECS, ids=["fp64", "fp32"])
def dev(request, emu_library):
    with gc.Dev(emu_library, 16, request.param, max_rows=16) as d:
        yield d


# ---- 1. the export -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("nrows,ncols,pattern", gc.CASES)
def test_adjoint_against_the_closed_form(dev, nrows, ncols, pattern, mode):
    gc.check_closed_form(dev, nrows, ncols, pattern, mode)


@pytest.mark.parametrize("mode", gc.MODES)
def test_the_forward_drops_the_planted_entries_too(dev, mode):
    gc.check_forward_agrees_on_planted(dev, mode)


@pytest.mark.parametrize("ncols", (1, 257, 2049, 4099))
@pytest.mark.parametrize("nrows", gc.ROWS)
def test_transpose_pair_of_the_linear_case(dev, nrows, ncols):
    gc.check_transpose(dev, nrows, ncols)


@pytest.mark.parametrize("mode", gc.MODES)
def test_in_place_gives_the_bits_of_out_of_place(dev, mode):
    gc.check_inplace(dev, mode)


@pytest.mark.parametrize("mode", gc.MODES)
def test_a_row_does_not_depend_on_its_neighbours_or_the_split(dev, mode):
    gc.check_independence(dev, mode)


def test_special_entries(dev):
    gc.check_special_entries(dev)


def test_refusals_touch_nothing(dev):
    codes, untouched = gc.refusals(dev)
    assert all(rc == gc.EINVAL for _, rc in codes), [c for c in codes if c[1] != gc.EINVAL]
    assert len(codes) >= 17 and untouched


@pytest.mark.parametrize("prec", gc.PRECS)
def test_the_call_between_its_siblings_on_a_live_plan(emu_library, prec):
    gc.check_live_plan_sequence(emu_library, prec)


# ---- 2. torch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (None, 3), ids=["one", "batch3"])
@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("name", gc.TORCH_MOTHERS)
def test_forward_is_denoise_and_icwt(emulated, name, prec, batch):
    gc.check_torch_forward(torch, CPU, name, prec, batch)


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("batch", (None, 3), ids=["one", "batch3"])
@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("name", gc.TORCH_MOTHERS)
def test_gradients_are_those_of_the_path_that_keeps_w(emulated, name, prec, batch, mode):
    gc.check_torch_gradients(torch, CPU, name, prec, batch, mode)


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("prec", gc.PRECS)
def test_w_grad_is_the_export(emulated, prec, mode):
    gc.check_w_grad_is_the_export(torch, CPU, emulated, prec, mode)


def test_gradcheck(emulated):
    gc.check_gradcheck(torch, CPU)


@pytest.mark.parametrize("mode", ("soft", "garrote"))
def test_central_difference_of_denoise_torch(emulated, mode):
    gc.check_central_difference(torch, CPU, mode)


def test_refusals_of_the_torch_entry_points(emulated):
    gc.check_torch_refusals(torch, CPU)


def test_a_non_finite_signal_gives_nan(emulated):
    gc.check_nonfinite_signal(torch, CPU)


# ---- 3. documents ------------------------------------------------------------------------------------------------------------------
def test_header_records_and_exports():
    import pycwt_amd
    text = open(os.path.join(ROOT, "include", "cwt_hip.h")).read()
    assert "int cwt_icwt_shrink_adjoint(" in text
    for name in ("icwt_torch", "icwt_shrink_torch", "denoise_torch"):
        assert name in pycwt_amd.__all__ and callable(getattr(pycwt_amd, name))
    for f in ("shrink_grad_kernel_resources.txt", "shrink_grad_accuracy.txt", "shrink_grad_bench.txt"):
        assert os.path.exists(os.path.join(ROOT, "profiles", f)), f
    assert "71 exports" in open(os.path.join(ROOT, "README.md")).read() and "71 exports" in open(os.path.join(ROOT, "DESIGN.md")).read()
