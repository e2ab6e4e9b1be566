"""The differentiable synchrosqueezed transform on the CPU emulation of the kernels (tests/emu): cwt_ssq_reassign_bins,
cwt_ssq_gather and the torch entry points ssq_cwt_torch / issq_cwt_torch.  The cases are in tests/ssq_grad_common.py; the same
ones run on the GPU in tests/test_ssq_grad_gpu.py."""
import os

import numpy as np
import pytest

import ssq_common as sc
import ssq_grad_common as gc
from conftest import ROOT

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", params=sc.PRECS, ids=["fp64", "fp32"])
def dev(request, emu_library):
    with sc.Dev(emu_library, 16, request.param, max_rows=64) as d:
        yield d


@pytest.fixture()
def engines(emulated, monkeypatch):
    from pycwt_amd import autograd
    monkeypatch.setattr(autograd, "_engines", {})
    yield autograd
    for eng in autograd._engines.values():
        eng.plan.close()


# ---- 1. cwt_ssq_reassign_bins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", gc.NFS)
@pytest.mark.parametrize("ncols", gc.NCOLS)
@pytest.mark.parametrize("rows", gc.ROWS)
def test_reassign_bins(dev, rows, ncols, nf):
    gc.check_reassign_bins(dev, rows, ncols, nf, chunkings=(None, 1, 5))


def test_reassign_bins_on_the_largest_grid(dev):
    gc.check_reassign_bins(dev, 9, gc.BIG_NF[1], gc.BIG_NF[0], chunkings=(None, 5))


def test_reassign_bins_accumulates_like_reassign(dev):
    gc.check_accumulate_adds(dev)


def test_reassign_bins_refusals_launch_nothing_and_touch_nothing(dev, emu_library):
    dev.plan.sync()
    emu_library.dll.hipemu_clear_launched()
    codes, untouched = gc.reassign_bins_refusals(dev)
    assert all(rc == gc.EINVAL for _, rc in codes), [c for c in codes if c[1] != gc.EINVAL]
    assert len(codes) >= 31 and untouched
    assert not sc.launch_log(emu_library), sc.launch_log(emu_library)


# ---- 2. cwt_ssq_gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", gc.NFS)
@pytest.mark.parametrize("ncols", gc.NCOLS)
@pytest.mark.parametrize("rows", gc.ROWS)
def test_gather(dev, rows, ncols, nf):
    gc.check_gather(dev, rows, ncols, nf)


def test_gather_on_the_largest_grid(dev):
    gc.check_gather(dev, 9, gc.BIG_NF[1], gc.BIG_NF[0])


def test_gather_over_more_stretches_of_rows_than_one_launch_takes(emu_library):
    """rows beyond 8 x 32768: the second slab of gridDim.y, its first stretch and a last one of 3 rows"""
    rows = 8 * 32768 + 11
    with sc.Dev(emu_library, 16, 64, max_rows=rows) as d:
        rng = np.random.default_rng(1)
        bins = rng.integers(-1, 5, size=(rows, 2)).astype(np.int16)
        gT, bins, w = gc.gather_inputs(3, bins, 5, 64, poison=False)
        G, guard = gc.run_gather(d, gT, bins, w)
        gc.assert_gather(G, guard, gT, bins, w, d.real)


def test_gather_refusals_launch_nothing_and_touch_nothing(dev, emu_library):
    dev.plan.sync()
    emu_library.dll.hipemu_clear_launched()
    codes, untouched = gc.gather_refusals(dev)
    assert all(rc == gc.EINVAL for _, rc in codes), [c for c in codes if c[1] != gc.EINVAL]
    assert len(codes) >= 17 and untouched
    assert not sc.launch_log(emu_library), sc.launch_log(emu_library)


# ---- 3. the pair is a transpose pair -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,ncols,nf", [(1, 1, 1), (9, 129, 5), (24, 300, 5), (13, 3, 32767)])
def test_transpose_identity(dev, rows, ncols, nf):
    gc.check_transpose(dev, rows, ncols, nf)


# ---- 5. ssq_cwt_torch, forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 3], ids=["one", "batch3"])
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(gc.TORCH_MOTHERS))
@pytest.mark.parametrize("n0", [1000, (1 << 15) - 77])
def test_torch_forward(engines, n0, name, prec, batch):
    gc.check_torch_forward(torch, "cpu", n0, name, prec, batch)


def test_torch_refusals(engines):
    gc.check_torch_refusals(torch, "cpu")


def test_nonfinite_signal_gives_nan_in_tx_and_gradient(engines):
    gc.check_nonfinite_signal(torch, "cpu")


def test_nothing_but_the_map_is_saved(engines):
    import pycwt_amd
    x = torch.tensor(gc.signal(300, 1, 64), requires_grad=True)
    Tx = pycwt_amd.ssq_cwt_torch(x, 1.0)[0]
    saved = Tx.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.int16 and saved[0] is engines._ssq_saved_bins(Tx)
    with pytest.raises(ValueError):
        engines._ssq_saved_bins(pycwt_amd.ssq_cwt_torch(x.detach(), 1.0)[0])
    with pytest.raises(ValueError):
        engines._ssq_saved_bins(Tx * 2)


# ---- 6. ssq_cwt_torch, backward: the exact route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, 3], ids=["one", "batch3"])
@pytest.mark.parametrize("prec", sc.PRECS)
@pytest.mark.parametrize("name", list(gc.TORCH_MOTHERS))
def test_torch_backward_is_the_adjoint_of_the_gathered_cotangent(engines, name, prec, batch):
    gc.check_torch_backward_exact(torch, "cpu", 1000, name, prec, batch)


# ---- 7. ssq_cwt_torch, backward: the independent route -----------------------------------------------------------------------------
def test_torch_backward_against_a_finite_difference_on_a_fixed_map(engines):
    for err, unit, an in gc.torch_independent_route(torch, "cpu", gc.INDEPENDENT_SEEDS):
        print("independent route: error", err, "unit eps sum|C||T| / h", unit, "ratio", err / unit, "<x.grad, dx>", an)
        assert err <= gc.INDEPENDENT_MARGIN * gc.INDEPENDENT_CONSTANT * unit


def test_issq_torch(engines):
    gc.check_issq_torch(torch, "cpu")


def test_the_exports_are_new():
    """the header declares both calls, and the kernels live in their own file"""
    text = open(os.path.join(ROOT, "include", "cwt_hip.h")).read()
    assert "int cwt_ssq_reassign_bins(" in text and "int cwt_ssq_gather(" in text
    assert os.path.exists(os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_ssq_grad.hpp"))
