"""The cases of tests/ssq_grad_common.py on the GPU: cwt_ssq_reassign_bins, cwt_ssq_gather and the torch entry points
ssq_cwt_torch / issq_cwt_torch, in both precisions, at the shapes of tests/test_ssq_grad_emulated.py plus the ones only a GPU
makes cheap (65539 rows against the slabs of gridDim.y; 2^18 samples x 64 scales) and a stream that is not the default one."""
import numpy as np
import pytest

import ssq_common as sc
import ssq_grad_common as gc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEVICE = "cuda"


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, hip_library):
    with sc.Dev(hip_library, 16, request.param, max_rows=64) as d:
        yield d


@pytest.fixture()
def engines(hip_library):
    """the engines of the torch entry points and the shim's plans of this test, closed when it ends"""
    import pycwt_amd
    from pycwt_amd import autograd, wavelet
    keep = autograd._engines
    autograd._engines = {}
    yield autograd
    torch.cuda.synchronize()
    for eng in autograd._engines.values():
        eng.plan.close()
    autograd._engines = keep
    for p in wavelet._plans.values():
        p.close()
    wavelet._plans.clear()
    pycwt_amd.release_scratch()


# ---- 1. cwt_ssq_reassign_bins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", gc.NFS)
@pytest.mark.parametrize("rows", gc.ROWS)
def test_reassign_bins(dev, rows, nf):
    for ncols in gc.NCOLS:
        gc.check_reassign_bins(dev, rows, ncols, nf, chunkings=(None, 1, 5))


def test_reassign_bins_on_the_largest_grid(dev):
    gc.check_reassign_bins(dev, 9, gc.BIG_NF[1], gc.BIG_NF[0], chunkings=(None, 5))


def test_reassign_bins_accumulates_like_reassign(dev):
    gc.check_accumulate_adds(dev)


def test_reassign_bins_refusals_touch_nothing(dev):
    codes, untouched = gc.reassign_bins_refusals(dev)
    assert all(rc == gc.EINVAL for _, rc in codes), [c for c in codes if c[1] != gc.EINVAL]
    assert len(codes) >= 31 and untouched


# ---- 2. cwt_ssq_gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", gc.NFS)
@pytest.mark.parametrize("rows", gc.ROWS)
def test_gather(dev, rows, nf):
    for ncols in gc.NCOLS:
        gc.check_gather(dev, rows, ncols, nf)


def test_gather_on_the_largest_grid(dev):
    gc.check_gather(dev, 9, gc.BIG_NF[1], gc.BIG_NF[0])


@pytest.mark.parametrize("rows", [65539, 8 * 32768 + 11])
def test_gather_over_many_stretches_of_rows(hip_library, rows):
    """65539 rows x 5 columns: 8193 stretches of rows in gridDim.y; beyond 8 x 32768 rows: the second launch over the slabs"""
    with sc.Dev(hip_library, 16, 64, max_rows=rows) as d:
        bins = np.random.default_rng(1).integers(-1, 5, size=(rows, 5)).astype(np.int16)
        gT, bins, w = gc.gather_inputs(3, bins, 5, 64, poison=False)
        G, guard = gc.run_gather(d, gT, bins, w)
        gc.assert_gather(G, guard, gT, bins, w, d.real)


def test_gather_refusals_touch_nothing(dev):
    codes, untouched = gc.gather_refusals(dev)
    assert all(rc == gc.EINVAL for _, rc in codes), [c for c in codes if c[1] != gc.EINVAL]
    assert len(codes) >= 17 and untouched


# ---- 3. the pair is a transpose pair -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,ncols,nf", [(1, 1, 1), (9, 129, 5), (24, 300, 5), (13, 3, 32767)])
def test_transpose_identity(dev, rows, ncols, nf):
    gc.check_transpose(dev, rows, ncols, nf)


# ---- 5. - 7. the torch entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 3], ids=["one", "batch3"])
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(gc.TORCH_MOTHERS))
@pytest.mark.parametrize("n0", [1000, (1 << 15) - 77])
def test_torch_forward(engines, n0, name, prec, batch):
    gc.check_torch_forward(torch, DEVICE, n0, name, prec, batch)


def test_torch_refusals(engines):
    gc.check_torch_refusals(torch, DEVICE)


def test_nonfinite_signal_gives_nan_in_tx_and_gradient(engines):
    gc.check_nonfinite_signal(torch, DEVICE)


@pytest.mark.parametrize("batch", [None, 3], ids=["one", "batch3"])
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(gc.TORCH_MOTHERS))
def test_torch_backward_is_the_adjoint_of_the_gathered_cotangent(engines, name, prec, batch):
    gc.check_torch_backward_exact(torch, DEVICE, 1000, name, prec, batch)


def test_torch_backward_against_a_finite_difference_on_a_fixed_map(engines):
    for err, unit, an in gc.torch_independent_route(torch, DEVICE, gc.INDEPENDENT_SEEDS):
        print("independent route: error", err, "unit eps sum|C||T| / h", unit, "ratio", err / unit, "<x.grad, dx>", an)
        assert err <= gc.INDEPENDENT_MARGIN * gc.INDEPENDENT_CONSTANT * unit


def test_issq_torch(engines):
    gc.check_issq_torch(torch, DEVICE)


# ---- 8. only on the device ---------------------------------------------------------------------------------------------------------
def test_forward_and_backward_on_a_side_stream(engines):
    gc.check_torch_stream(torch, DEVICE)


def test_torch_large(engines):
    gc.check_torch_large(torch, DEVICE)
