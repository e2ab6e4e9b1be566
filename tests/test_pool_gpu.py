"""The time-pooled scalogram (cwt_transform_pool, the `pool=` keyword) on a real MI355X: the every-form, (K', D), short-signal,
determinism and autograd cases of tests/test_pool_emulated.py at the same shapes through the built library, with the same
references and bounds (tests/pool_common.py, profiles/pool_accuracy.txt: 4 x the ratio measured on the emulation, 1.826e-15 /
1.096e-06), and one case at the bench's own shape."""
import numpy as np
import pytest

import pool_common as pc
import pycwt_amd
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND as ADJOINT_BOUND
from test_kernels_emulated import grid

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N20 = 1 << 20


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("form", pc.FORMS, ids=[f[0] for f in pc.FORMS])
def test_every_row_form_pooled_equals_the_pooled_power_on_the_device(hip_library, form, prec):
    pc.check_form(hip_library, form, prec, pc.BOUND[prec])


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("tolerance", [pc.POLY_TOLERANCE, 0.0], ids=["tol1e-9", "round-off"])
def test_polynomial_rows_by_interval_count_and_degree_on_the_device(hip_library, tolerance, prec):
    pc.check_poly_rows(hip_library, prec, tolerance, pc.BOUND[prec], want=pc.WANT if tolerance else None)


@pytest.mark.parametrize("prec", [64, 32])
def test_short_signal_and_oracle_on_the_device(hip_library, prec):
    pc.check_short_signal(hip_library, prec, pc.BOUND[prec])
    N, n0, sj, x, Pref = pc.oracle_case(prec)
    peak = Pref.max(axis=1)
    with pc.Device(hip_library, N, prec, max_rows=len(sj), options={"poly_min_logn": 14, "ols_min_logn": 15}) as dev:
        for pool in (2, 64, 4096):
            B = pc.run_pool(dev, x, pc.MORLET, pc.F0, sj, pool)
            err = (np.abs(B.astype(np.longdouble) - pc.window_means(Pref, pool)).max(axis=1) / peak).max()
            assert err <= pc.ORACLE_BOUND[prec], (pool, float(err))


@pytest.mark.parametrize("prec", [64, 32])
def test_bits_do_not_depend_on_the_batch_the_run_or_the_calls_around_on_the_device(hip_library, prec):
    N, n0, pool = 1 << 15, (1 << 15) - 77, 64
    sj = grid(n0, 1.0, orc.Mother(pc.MORLET, pc.F0), 40)
    rows = len(sj)
    X = np.random.default_rng(31).standard_normal((3, n0))
    with pc.Device(hip_library, N, prec, max_rows=3 * rows, options={"poly_min_logn": 14, "ols_min_logn": 15}) as dev:
        xd, Wd = dev.up(X[1].astype(dev.real)), dev.up(np.zeros((rows, n0), dtype=dev.cplx))
        dev.plan.transform(xd.ptr, n0, pc.MORLET, pc.F0, 1.0, sj, None, Wd.ptr, n0, n0)
        W0, split = Wd.download(dev.plan, (rows, n0), dev.cplx), dev.plan.last_split()
        one = pc.run_pool(dev, X[1], pc.MORLET, pc.F0, sj, pool)
        assert dev.plan.last_split() == split
        dev.plan.transform(xd.ptr, n0, pc.MORLET, pc.F0, 1.0, sj, None, Wd.ptr, n0, n0)
        assert np.array_equal(Wd.download(dev.plan, (rows, n0), dev.cplx).view(np.uint8), W0.view(np.uint8))
        assert np.array_equal(one.view(np.uint8), pc.run_pool(dev, X[1], pc.MORLET, pc.F0, sj, pool).view(np.uint8))
        batch = pc.run_pool(dev, X, pc.MORLET, pc.F0, sj, pool)
        assert np.array_equal(batch[rows:2 * rows].view(np.uint8), one.view(np.uint8))


def test_bench_shape_against_the_window_means_of_the_power(hip_library):
    """N = 2^20, 256 scales, fp64 Morlet at 1e-9, pool 256: the classifier runs as bench.py runs it and pool_poly_rows meets its
    real grid and chunking; compared on the device against the window means of cwt_transform_power on the same plan, only the
    per-row error downloaded.  The reference's own sum is made exact: every value is split at 2^-26 of its window's largest power of
    two, the high parts (27 bits each, 256 of them) add without rounding in float64, the low parts are 2^-26 of the window."""
    pool, rows = 256, 256
    m = orc.Mother(pc.MORLET, pc.F0)
    s0 = 2.0 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(N20 / s0) / (rows - 1))
    n0, nc = N20, N20 // pool
    gen = torch.Generator(device="cuda").manual_seed(47)
    x = torch.randn(n0, dtype=torch.float64, device="cuda", generator=gen)
    P = torch.empty((rows, n0), dtype=torch.float64, device="cuda")
    Pb = torch.full((rows, nc), pc.SENTINEL, dtype=torch.float64, device="cuda")
    plan = _hip.Plan(N20, 64, max_rows=rows, lib=hip_library, options={"tolerance": 1e-9})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        plan.transform_power(x.data_ptr(), n0, pc.MORLET, pc.F0, 1.0, sj, None, P.data_ptr(), n0, n0)
        split = plan.last_split()
        plan.transform_pool(x.data_ptr(), 1, n0, n0, pc.MORLET, pc.F0, 1.0, sj, pool, None, Pb.data_ptr(), nc)
        torch.cuda.synchronize()
        assert plan.last_split() == split and split["poly"] > rows // 2, split
    finally:
        plan.close()
    Pw = P.reshape(rows, nc, pool)
    q = torch.exp2(torch.ceil(torch.log2(Pw.amax(dim=2, keepdim=True))) - 26)
    hi = torch.round(Pw / q) * q
    ref = (hi.sum(dim=2) + (Pw - hi).sum(dim=2)) / pool
    err = ((Pb - ref).abs().amax(dim=1) / ref.amax(dim=1)).max().item()
    print("2^20 x 256, pool 256: pooled rows against the window means of the power", err, "bound", pc.BOUND[64], "split", split)
    assert err <= pc.BOUND[64], (err, pc.BOUND[64])


def test_gradcheck_on_the_device(hip_library):
    x = torch.randn((2, 500), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 2.0, wavelet="dog", pool=4)[0], (x,), atol=1e-8)


def window_mean_torch(P, pool):
    n0 = P.shape[-1]
    nc = -(-n0 // pool)
    padded = torch.nn.functional.pad(P, (0, nc * pool - n0))
    count = torch.full((nc,), float(pool), dtype=P.dtype, device=P.device)
    count[-1] = n0 - (nc - 1) * pool
    return padded.reshape(P.shape[:-1] + (nc, pool)).sum(dim=-1) / count


@pytest.mark.parametrize("prec", [64, 32])
def test_gradient_against_the_explicit_window_mean_on_the_device(hip_library, prec):
    """N = 2^15, ragged n0, pool 64: x.grad through cwt_power_torch(pool=) against cwt_power_torch + a window mean in torch (BOUND
    of test_adjoint_emulated); with scales= and f0= (fp64) the three gradients the same way."""
    real_t = torch.float64 if prec == 64 else torch.float32
    n0, pool = (1 << 15) - 77, 64
    gen = torch.Generator(device="cuda").manual_seed(45)
    x0 = torch.randn(n0, dtype=real_t, device="cuda", generator=gen)
    xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    P = pycwt_amd.cwt_power_torch(xa, 1.0, 1 / 4, wavelet="morlet")[0]
    Pp, _, _, coi = pycwt_amd.cwt_power_torch(xb, 1.0, 1 / 4, wavelet="morlet", pool=pool)
    ref = window_mean_torch(P, pool)
    assert Pp.shape == ref.shape and coi.shape == (Pp.shape[-1],)
    assert pc.row_ratio(Pp.detach().cpu().numpy(), pc.window_means(P.detach().cpu().numpy(), pool)).max() <= pc.BOUND[prec]
    gP = torch.randn(Pp.shape, dtype=real_t, device="cuda", generator=gen)
    (ref * gP).sum().backward()
    (Pp * gP).sum().backward()
    torch.cuda.synchronize()
    a, b = xa.grad.double().cpu().numpy(), xb.grad.double().cpu().numpy()
    err = np.linalg.norm(b - a) / np.linalg.norm(a)
    print("pooled gradient against the explicit window mean, precision", prec, err)
    assert err <= ADJOINT_BOUND[prec], err
    if prec == 32:
        return
    grads = []
    t0 = torch.as_tensor(2.0 * 2 ** (np.arange(10) * 0.9))
    for pooled in (False, True):
        x, t = x0[:4019].clone().requires_grad_(True), t0.clone().requires_grad_(True)
        f0 = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
        if pooled:
            out = pycwt_amd.cwt_power_torch(x, 1.0, wavelet="morlet", scales=t, f0=f0, pool=16)[0]
        else:
            out = window_mean_torch(pycwt_amd.cwt_power_torch(x, 1.0, wavelet="morlet", scales=t, f0=f0)[0], 16)
        if not grads:
            g = torch.randn(out.shape, dtype=torch.float64, device="cuda", generator=gen)
        (out * g).sum().backward()
        grads.append([v.grad.double().cpu().numpy().reshape(-1) for v in (x, t, f0)])
    for u, v in zip(*grads):
        assert np.linalg.norm(v - u) <= ADJOINT_BOUND[64] * np.linalg.norm(u)
