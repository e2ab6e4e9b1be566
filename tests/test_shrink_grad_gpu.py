"""The cases of tests/shrink_grad_common.py on the GPU: cwt_icwt_shrink_adjoint and the torch entry points icwt_torch,
icwt_shrink_torch and denoise_torch in both precisions, at the shapes of tests/test_shrink_grad_emulated.py, plus what only a
device shows: rows of 2^17 + 3 columns (65 slices a row), torch's memory counter and a stream that is not the default one."""
import pytest

import pycwt_amd
import shrink_grad_common as gc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", params=gc.PRECS, ids=["fp64", "fp32"])
def dev(request, hip_library):
    with gc.Dev(hip_library, 16, request.param, max_rows=16) as d:
        yield d


@pytest.fixture()
def gpu(hip_library):
    """the device of the torch cases; the shim's plans of the test are closed when it ends"""
    from pycwt_amd import wavelet
    assert torch.cuda.is_available()
    yield torch.device("cuda", 0)
    for p in wavelet._plans.values():
        p.close()
    wavelet._plans.clear()
    pycwt_amd.release_scratch()


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("nrows,ncols,pattern", gc.CASES)
def test_adjoint_against_the_closed_form(dev, nrows, ncols, pattern, mode):
    gc.check_closed_form(dev, nrows, ncols, pattern, mode)


@pytest.mark.parametrize("mode", gc.MODES)
def test_one_row_over_65_slices(hip_library, mode):
    gc.check_large(hip_library, mode)


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
def test_the_call_between_its_siblings_on_a_live_plan(hip_library, prec):
    gc.check_live_plan_sequence(hip_library, prec)


@pytest.mark.parametrize("batch", (None, 3), ids=["one", "batch3"])
@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("name", gc.TORCH_MOTHERS)
def test_forward_is_denoise_and_icwt(gpu, name, prec, batch):
    gc.check_torch_forward(torch, gpu, name, prec, batch)


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("batch", (None, 3), ids=["one", "batch3"])
@pytest.mark.parametrize("prec", gc.PRECS)
@pytest.mark.parametrize("name", gc.TORCH_MOTHERS)
def test_gradients_are_those_of_the_path_that_keeps_w(gpu, name, prec, batch, mode):
    gc.check_torch_gradients(torch, gpu, name, prec, batch, mode)


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("prec", gc.PRECS)
def test_w_grad_is_the_export(gpu, hip_library, prec, mode):
    gc.check_w_grad_is_the_export(torch, gpu, hip_library, prec, mode)


def test_gradcheck(gpu):
    gc.check_gradcheck(torch, gpu)


@pytest.mark.parametrize("mode", ("soft", "garrote"))
def test_central_difference_of_denoise_torch(gpu, mode):
    gc.check_central_difference(torch, gpu, mode)


def test_refusals_of_the_torch_entry_points(gpu):
    gc.check_torch_refusals(torch, gpu)


def test_a_non_finite_signal_gives_nan(gpu):
    gc.check_nonfinite_signal(torch, gpu)


def test_denoise_torch_holds_nothing_of_the_size_of_w(gpu):
    gc.check_torch_memory(torch, gpu)


def test_a_side_stream_gives_the_bits_of_the_default_stream(gpu):
    gc.check_torch_stream(torch, gpu)
