"""The adjoint of the row transform (cwt_adjoint_rows) and cwt_torch's backward on the MI355X: the config-2 workload
(N = 2^20, 256 scales) through the adjoint identity and against an FFT-based NumPy adjoint, torch's gradcheck on the device,
the bits of a backward on another stream, and the transpose of the polynomial form against the general path."""
import numpy as np
import pytest

from oracle import cwt_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N20 = 1 << 20
ROUNDOFF, BENCH_TAU = {64: 0.0, 32: 0.0}, {64: 1e-9, 32: 3e-5}


def c2_grid(m, n=N20, rows=256):
    """bench.py's scale grid: s0 = 2 dt / flambda, 256 scales up to n dt, without the rows the reference drops."""
    s0 = 2.0 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(n / s0) / (rows - 1))
    return sj[~orc.dropped_rows(sj, 1.0, m)]


def plan_for(hip_library, prec, rows, tol, options=None):
    from pycwt_amd import _hip
    plan = _hip.Plan(N20, prec, max_rows=rows, lib=hip_library, options=options)
    plan.set_tolerance(tol)
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    return plan


def forward_and_adjoint(plan, kind, param, sj, x, G):
    n0 = x.shape[0]
    W = torch.empty((sj.size, n0), dtype=G.dtype, device="cuda")
    plan.transform(x.data_ptr(), n0, kind, param, 1.0, sj, None, W.data_ptr(), n0, n0)
    xbar = torch.empty(n0, dtype=x.dtype, device="cuda")
    plan.adjoint_rows(G.data_ptr(), 1, sj.size * n0, n0, n0, kind, param, 1.0, sj, xbar.data_ptr(), n0)
    torch.cuda.synchronize()
    return W, xbar


def numpy_adjoint(G, sj, m, N, slab=16):
    """Re (1/N) DFT^H( sum_j conj(F_j) DFT(pad G_j) ), the filters a slab of rows at a time (a full bank is 4 GB at c2)."""
    w = orc.angular_freqs(N, 1.0)
    acc = np.zeros(N, dtype=np.complex128)
    for j0 in range(0, len(sj), slab):
        bank = orc.filter_bank(np.asarray(sj[j0:j0 + slab], dtype=float), w, N, m, True)
        acc += (np.conj(bank) * np.fft.fft(G[j0:j0 + slab], n=N, axis=1)).sum(axis=0)
    return np.real(np.fft.ifft(acc))[:G.shape[1]]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("kind,param,prec", [(orc.MORLET, 6, 64), (orc.PAUL, 4, 64), (orc.DOG, 2, 64), (orc.DOG, 2, 32)])
def test_c2_adjoint_identity_and_numpy_adjoint(hip_library, kind, param, prec):
    """c2 geometry (N = 2^20, 256 scales, n0 = N - 1000), at round-off and at bench.py's target: Re <G, A x> = <x, A^H G> and
    xbar against the NumPy adjoint."""
    m = orc.Mother(kind, param)
    n0 = N20 - 1000
    sj = c2_grid(m)
    rng = np.random.default_rng(11)
    real_t, cplx_t = (torch.float64, torch.complex128) if prec == 64 else (torch.float32, torch.complex64)
    x_h = rng.standard_normal(n0)
    G_h = rng.standard_normal((sj.size, n0)) + 1j * rng.standard_normal((sj.size, n0))
    x = torch.as_tensor(x_h, dtype=real_t, device="cuda")
    G = torch.as_tensor(G_h, dtype=cplx_t, device="cuda")
    ref = numpy_adjoint(G.cpu().numpy().astype(np.complex128), sj, m, N20)
    for tol, bound, ident in ((ROUNDOFF[prec], {64: 1e-12, 32: 1e-5}[prec], {64: 1e-12, 32: 1e-5}[prec]),
                              (BENCH_TAU[prec], {64: 1e-8, 32: 3e-4}[prec], {64: 1e-8, 32: 3e-4}[prec])):
        plan = plan_for(hip_library, prec, sj.size, tol)
        W, xbar = forward_and_adjoint(plan, kind, float(param), sj, x, G)
        classes = plan.row_classes()
        plan.close()
        xb = xbar.cpu().numpy().astype(np.float64)
        lhs = float(torch.real(torch.vdot(G.reshape(-1).to(torch.complex128), W.reshape(-1).to(torch.complex128))))
        rhs = float(np.dot(x.cpu().numpy().astype(np.float64), xb))
        scale = float(torch.linalg.vector_norm(G.to(torch.complex128))) * float(torch.linalg.vector_norm(W.to(torch.complex128)))
        assert abs(lhs - rhs) <= ident * scale, (tol, lhs, rhs, classes[:4])
        assert rel(xb, ref) <= bound, (tol, rel(xb, ref))


def test_polynomial_transpose_against_the_general_path_on_c2(hip_library):
    """Every polynomial row of c2 (fp64 Morlet at bench.py's target), alone in G: adjoint_poly = 1 against adjoint_poly = 0."""
    m = orc.Mother(orc.MORLET, 6)
    sj = c2_grid(m)
    n0 = N20
    plan = plan_for(hip_library, 64, sj.size, 1e-9)
    classes = plan.classify(orc.MORLET, 6.0, 1.0, sj, n0, True)
    poly = np.array([c.startswith("poly") for c in classes])
    assert poly.sum() >= 100, classes
    rng = np.random.default_rng(5)
    G_h = (rng.standard_normal((sj.size, n0)) + 1j * rng.standard_normal((sj.size, n0))) * poly[:, None]
    G = torch.as_tensor(G_h, dtype=torch.complex128, device="cuda")
    out = []
    for flag in (1, 0):
        plan.set_option("adjoint_poly", flag)
        xbar = torch.empty(n0, dtype=torch.float64, device="cuda")
        plan.adjoint_rows(G.data_ptr(), 1, sj.size * n0, n0, n0, orc.MORLET, 6.0, 1.0, sj, xbar.data_ptr(), n0)
        torch.cuda.synchronize()
        out.append(xbar.cpu().numpy())
    plan.close()
    assert not np.array_equal(out[0], out[1])
    assert rel(out[0], out[1]) <= 1e-8, rel(out[0], out[1])


def test_gradcheck_on_the_device(hip_library):
    import pycwt_amd
    x = torch.randn(1 << 10, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_torch(t, 1.0, 1 / 2, wavelet="morlet")[0], (x,), atol=1e-8,
                                    fast_mode=True)
    xb = torch.randn(2, 700, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_torch(t, 1.0, 1 / 2, wavelet="dog")[0], (xb,), atol=1e-8,
                                    fast_mode=True)


def test_backward_on_another_stream_gives_the_same_bits(hip_library):
    import pycwt_amd
    x0 = torch.randn(1 << 16, dtype=torch.float64, device="cuda")

    def grad():
        x = x0.clone().requires_grad_(True)
        W = pycwt_amd.cwt_torch(x, 1.0, 1 / 8, wavelet="morlet")[0]
        (W.abs() ** 2).sum().backward()
        return x.grad

    g0 = grad()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g1 = grad()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(g0, g1)
    W, sj, _, _ = pycwt_amd.cwt_torch(x0, 1.0, 1 / 8, wavelet="morlet")
    ref = pycwt_amd.cwt(x0.cpu().numpy(), 1.0, 1 / 8, wavelet="morlet")[0]
    np.testing.assert_allclose(W.cpu().numpy(), ref, rtol=0, atol=1e-12 * np.abs(ref).max())
