"""The weighted output (cwt_transform_weighted) and pycwt_amd.cwt_power_torch on a real MI355X: every row form against
alpha Q W of the same plan, the production instantiations of the config-2 and config-3 workloads at N = 2^20 (compared on the
device, nothing of rows x n0 elements downloaded), torch's gradcheck, the backward against the route through cwt_torch and on a
second stream, and what a forward allocates."""
import numpy as np
import pytest

import pycwt_amd
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND, rel
from test_kernels_emulated import grid
from test_power_emulated import EPS32, FORMS
from test_weighted_emulated import ALPHAS, outputs, weighted_bound

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N20 = 1 << 20


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("name,N,n0,kind,param,rows,opts,form", FORMS, ids=[f[0] for f in FORMS])
def test_every_row_form_weighted_on_the_device(hip_library, prec, name, N, n0, kind, param, rows, opts, form):
    x = np.random.default_rng(7).standard_normal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    W, Q, G, split = outputs(hip_library, N, x, kind, param, sj, prec, opts)
    form = form[prec] if isinstance(form, dict) else form
    assert split[form] > 0, split
    for alpha in ALPHAS:
        weighted_bound(G[alpha], W, Q, alpha, prec)


def bench_grid(m, n=N20, rows=256):
    """bench.py's scale grid: s0 = 2 dt / flambda, 256 scales up to n dt, without the rows the reference drops"""
    s0 = 2.0 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(n / s0) / (rows - 1))
    return sj[~orc.dropped_rows(sj, 1.0, m)]


@pytest.mark.parametrize("kind,param,prec,tau", [(orc.MORLET, 6, 64, 1e-9), (orc.DOG, 2, 32, 3e-5)], ids=["config2", "config3_dog"])
def test_production_instantiations_at_2_20(hip_library, kind, param, prec, tau):
    """The tiles and classes only the bench workloads reach (4096-point overlap-save tiles, pairs of 8192-point tiles,
    polynomial classes K' >= 4096, the paired complex64 blocks at 2^13): G against 2 Q W of the same plan, formed on the device
    in float64 in slabs of 32 rows; per row and per part max|dG| / max|2 Q W| <= 32 eps, only the per-row figures come back."""
    real_t, cplx_t = (torch.float64, torch.complex128) if prec == 64 else (torch.float32, torch.complex64)
    m = orc.Mother(kind, param)
    sj = bench_grid(m)
    rows, n0 = sj.size, N20
    gen = torch.Generator(device="cuda").manual_seed(41)
    x = torch.randn(n0, dtype=real_t, device="cuda", generator=gen)
    Q = torch.randn((rows, n0), dtype=real_t, device="cuda", generator=gen)
    Q[torch.rand((rows, n0), device="cuda", generator=gen) < 0.01] = 0
    W = torch.empty((rows, n0), dtype=cplx_t, device="cuda")
    G = torch.full((rows, n0), -7 - 7j, dtype=cplx_t, device="cuda")
    plan = _hip.Plan(N20, prec, max_rows=rows, lib=hip_library, options={"tolerance": tau})
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        plan.transform(x.data_ptr(), n0, kind, float(param), 1.0, sj, None, W.data_ptr(), n0, n0)
        split = plan.last_split()
        plan.transform_weighted(x.data_ptr(), n0, kind, float(param), 1.0, sj, None, Q.data_ptr(), 2.0, G.data_ptr(), n0, n0)
        assert plan.last_split() == split
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert split["ols"] > 0 and split["aols"] > 0 and split["poly"] > 0, split
    worst = 0.0
    for lo in range(0, rows, 32):
        ref = 2.0 * Q[lo:lo + 32].to(torch.float64) * W[lo:lo + 32].to(torch.complex128)
        got = G[lo:lo + 32].to(torch.complex128)
        for g, r in ((got.real, ref.real), (got.imag, ref.imag)):
            assert not bool(torch.isnan(g).any()) and not bool(torch.isnan(r).any())
            err = (g - r).abs().amax(dim=1) / r.abs().amax(dim=1).clamp_min(1e-300)
            worst = max(worst, float(err.max()))
    print("weighted output at N = 2^20, precision", prec, ": worst per-row error", worst, "bound", EPS32[prec])
    assert worst <= EPS32[prec], worst


def test_gradcheck_on_the_device(hip_library):
    x = torch.randn(48, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 1.0, wavelet="morlet")[0], (x,), atol=1e-8)


def test_backward_of_a_float32_batch_against_the_route_through_cwt_torch(hip_library):
    """(3, 4099) in complex64: the two routes differ by the rounding of G = 2 gP W (BOUND of test_adjoint_emulated)."""
    gen = torch.Generator(device="cuda").manual_seed(42)
    x0 = torch.randn((3, 4099), dtype=torch.float32, device="cuda", generator=gen)
    xa = x0.clone().requires_grad_(True)
    W = pycwt_amd.cwt_torch(xa, 1.0, 1 / 4, wavelet="dog")[0]
    gP = torch.randn(W.shape, dtype=torch.float32, device="cuda", generator=gen)
    (W.abs().pow(2) * gP).sum().backward()
    xb = x0.clone().requires_grad_(True)
    P = pycwt_amd.cwt_power_torch(xb, 1.0, 1 / 4, wavelet="dog")[0]
    assert P.dtype == torch.float32 and P.shape == W.shape
    (P * gP).sum().backward()
    torch.cuda.synchronize()
    err = rel(xb.grad.double().cpu().numpy(), xa.grad.double().cpu().numpy())
    print("float32 batch: gradient against the route through cwt_torch", err)
    assert err <= BOUND[32], err


def test_backward_on_another_stream_gives_the_same_bits(hip_library):
    x0 = torch.randn(1 << 16, dtype=torch.float64, device="cuda")
    gP = torch.randn(1, dtype=torch.float64, device="cuda")

    def grad():
        x = x0.clone().requires_grad_(True)
        P = pycwt_amd.cwt_power_torch(x, 1.0, 1 / 8, wavelet="morlet")[0]
        (P * gP).sum().backward()
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


def test_a_forward_of_config2_allocates_the_power_and_no_w(hip_library):
    """torch's allocation across one forward of config 2 (N = 2^20, 256 scales, fp64): at most P (8 rows n0 bytes) + a transient
    spectrum and slack (2 x 16 N) + 1 MiB of allocator rounding -- from the shapes; W alone would be 16 rows n0."""
    m = pycwt_amd.Morlet(6)
    rows = 256
    s0 = 2.0 / m.flambda()
    dj = np.log2(N20 / s0) / (rows - 1)
    x = torch.randn(N20, dtype=torch.float64, device="cuda", requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    P, sj, _, _ = pycwt_amd.cwt_power_torch(x, 1.0, dj, s0, rows - 1, m)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    peak = torch.cuda.max_memory_allocated() - before
    limit = 8 * sj.size * N20 + 2 * 16 * N20 + (1 << 20)
    print("forward of config 2: allocated", grown, "peak", peak, "limit", limit, "W alone", 16 * sj.size * N20)
    assert P.shape == (sj.size, N20) and sj.size == rows
    assert grown <= limit and peak <= limit, (grown, peak, limit)
    assert [tuple(t.shape) for t in P.grad_fn.saved_tensors] == [(N20,)]
