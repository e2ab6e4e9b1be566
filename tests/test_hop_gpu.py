"""The decimated transform (cwt_transform_hop, cwt_adjoint_rows_hop, the `hop=` keyword) on a real MI355X: the emulated W /
power / weighted cases at nfft = 2^12 and 2^16 with the same references and bounds (tests/hop_common.py,
profiles/hop_accuracy.txt: 4 x the measured error of the existing cwt_transform, 1.615e-14 / 3.423e-05), the flagship
length, the adjoint, torch's gradcheck, a second stream, and what torch allocates."""
import numpy as np
import pytest

import hop_common as hc
import pycwt_amd
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND as ADJOINT_BOUND, random_g
from test_hop_emulated import draw_q, run_adjoint
from test_power_emulated import EPS32

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N20 = 1 << 20
CASE_IDS = [hc.case_id(c) for c in hc.CASES]


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", hc.CASES, ids=CASE_IDS)
def test_hop_rows_against_the_oracle_power_and_weighted_on_the_device(hip_library, case, prec):
    """test_hop_emulated's values test on the device: HOP_BOUND against oracle[:, ::hop]; power = re^2 + im^2 to 4 eps of the
    value; weighted = (alpha Q) W_h within 32 eps of the row peak; fold kernel and fused fold agree to the bits."""
    logn, hop, n0, kind, param = case
    sj, ref, peak = hc.reference(logn, n0, kind, param, prec)
    x = hc.signal(n0, prec)
    eps = float(np.finfo(hc.types(prec)[0]).eps)
    with hc.Device(hip_library, 1 << logn, prec) as dev:
        W = hc.run_hop(dev, x, kind, param, sj, hop)
        err = hc.row_error(W, ref[:, ::hop], peak)
        print("hop rows against the oracle:", hc.case_id(case), prec, err, "bound", hc.HOP_BOUND[prec])
        assert err <= hc.HOP_BOUND[prec], (err, hc.HOP_BOUND[prec])
        P = hc.run_hop(dev, x, kind, param, sj, hop, output=1)
        Wd = W.astype(np.complex128)
        want = Wd.real ** 2 + Wd.imag ** 2
        assert np.all(np.abs(P.astype(np.float64) - want) <= 4 * eps * want)
        Q = draw_q(11, W.shape, dev.real)
        for alpha in (2.0, -0.75):
            G = hc.run_hop(dev, x, kind, param, sj, hop, output=2, Q=Q, alpha=alpha).astype(np.complex128)
            want = alpha * Q.astype(np.float64) * Wd
            for got, w in ((G.real, want.real), (G.imag, want.imag)):
                e = np.abs(got - w).max(axis=1) / np.where(np.abs(w).max(axis=1) == 0, 1.0, np.abs(w).max(axis=1))
                assert e.max() <= EPS32[prec], (alpha, e.max())
        dev.plan.set_option("hop_fuse_terms", 0)                      # every row through the fold kernel and scratch
        W0 = hc.run_hop(dev, x, kind, param, sj, hop)
        dev.plan.set_option("hop_fuse_terms", 65536)                  # ... and none
        W1 = hc.run_hop(dev, x, kind, param, sj, hop)
    assert np.array_equal(W0.view(np.uint8), W.view(np.uint8)) and np.array_equal(W1.view(np.uint8), W.view(np.uint8))


def bench_scales(m, rows, n=N20, total=256):
    """`rows` scales spread over bench.py's grid of config 2 (256 scales from the period 2 dt to n dt)"""
    s0 = 2.0 / m.flambda()
    sj = s0 * 2 ** (np.arange(total) * np.log2(n / s0) / (total - 1))
    return sj[np.linspace(0, total - 1, rows).round().astype(int)]


@pytest.mark.parametrize("kind,param,prec", [(orc.MORLET, 6, 64), (orc.DOG, 2, 32)], ids=["fp64_morlet", "fp32_dog"])
def test_flagship_length_against_the_existing_transform(hip_library, kind, param, prec):
    """nfft = 2^20, hop = 256, 32 scales spread over config 2's grid: against columns ::256 of the existing cwt_transform at
    round-off, compared on the device, per row relative to the row's peak.  Bound: the SUM of the two measured errors against
    the oracle (profiles/hop_accuracy.txt) -- the existing transform's 4.038e-15 / 8.556e-06 and the 4 x that of a hop row."""
    real_t, cplx_t = (torch.float64, torch.complex128) if prec == 64 else (torch.float32, torch.complex64)
    hop, n0 = 256, N20 - 77
    sj = bench_scales(orc.Mother(kind, param), 32)
    nch = -(-n0 // hop)
    gen = torch.Generator(device="cuda").manual_seed(43)
    x = torch.randn(n0, dtype=real_t, device="cuda", generator=gen)
    W = torch.empty((len(sj), n0), dtype=cplx_t, device="cuda")
    Wh = torch.full((len(sj), nch), -7 - 7j, dtype=cplx_t, device="cuda")
    plan = _hip.Plan(N20, prec, max_rows=64, lib=hip_library)
    plan.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        plan.transform(x.data_ptr(), n0, kind, float(param), 1.0, sj, None, W.data_ptr(), n0, n0)
        plan.transform_hop(x.data_ptr(), 1, n0, n0, kind, float(param), 1.0, sj, hop, None, 0, Wh.data_ptr(), nch)
        torch.cuda.synchronize()
    finally:
        plan.close()
    peak = W.abs().amax(dim=1).double()
    err = ((Wh - W[:, ::hop]).abs().amax(dim=1).double() / peak).max().item()
    bound = hc.EXISTING_ERROR[prec] + hc.HOP_BOUND[prec]
    print("2^20, hop 256, precision", prec, ": hop rows against the existing transform", err, "bound", bound)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("prec", [64, 32])
def test_adjoint_identity_on_the_device(hip_library, prec):
    """2^16, hop = 16: Re <G, A_h x> = <x, A_h^H G>, within hop_common.identity_bound; a batch bit-identical to single calls"""
    N, n0, hop, kind, param = 1 << 16, (1 << 16) - 77, 16, orc.DOG, 2
    sj = hc.scales(N, kind, param, 24)
    rng = np.random.default_rng(23)
    x = rng.standard_normal(n0)
    with hc.Device(hip_library, N, prec, max_rows=3 * len(sj)) as dev:
        Ax = hc.run_hop(dev, x, kind, param, sj, hop).astype(np.complex128)
        G = random_g(rng, 3, *Ax.shape).astype(dev.cplx)
        xbar = run_adjoint(dev, G, n0, hop, kind, param, sj)
        for b in range(3):
            assert np.array_equal(run_adjoint(dev, G[b:b + 1], n0, hop, kind, param, sj)[0].view(np.uint8), xbar[b].view(np.uint8))
    lhs = float(np.real(np.vdot(G[0].astype(np.complex128), Ax)))
    rhs = float(np.dot(x.astype(dev.real).astype(np.float64), xbar[0].astype(np.float64)))
    scale = max(np.linalg.norm(G[0]) * np.linalg.norm(Ax), np.linalg.norm(x) * np.linalg.norm(xbar[0]))
    assert abs(lhs - rhs) <= hc.identity_bound(ADJOINT_BOUND, prec) * scale, (lhs, rhs)


def test_gradcheck_on_the_device(hip_library):
    x = torch.randn(131, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_torch(t, 0.5, 2.0, wavelet="morlet", hop=4)[0], (x,), atol=1e-8)
    xb = torch.randn((2, 129), dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 2.0, wavelet="dog", hop=4)[0], (xb,), atol=1e-8)


def test_gradient_against_the_existing_route_on_the_device(hip_library):
    """fp32 batch (3, 2^15 - 77), hop = 16: the gradient of a loss on P[:, :, ::h] through the existing cwt_power_torch against
    cwt_power_torch(hop=h); the two routes hand the adjoint the same G up to rounding (BOUND of test_adjoint_emulated)."""
    gen = torch.Generator(device="cuda").manual_seed(44)
    hop = 16
    x0 = torch.randn((3, (1 << 15) - 77), dtype=torch.float32, device="cuda", generator=gen)
    xa = x0.clone().requires_grad_(True)
    P = pycwt_amd.cwt_power_torch(xa, 1.0, 1 / 4, wavelet="dog")[0]
    xb = x0.clone().requires_grad_(True)
    Ph, _, _, coi = pycwt_amd.cwt_power_torch(xb, 1.0, 1 / 4, wavelet="dog", hop=hop)
    assert Ph.shape == P[:, :, ::hop].shape and coi.shape == (Ph.shape[-1],)
    gP = torch.randn(Ph.shape, dtype=torch.float32, device="cuda", generator=gen)
    (P[:, :, ::hop] * gP).sum().backward()
    (Ph * gP).sum().backward()
    torch.cuda.synchronize()
    a, b = xa.grad.double().cpu().numpy(), xb.grad.double().cpu().numpy()
    err = np.linalg.norm(b - a) / np.linalg.norm(a)
    print("float32 batch: hop gradient against the existing route", err)
    assert err <= ADJOINT_BOUND[32], err


def test_backward_on_another_stream_gives_the_same_bits(hip_library):
    x0 = torch.randn((1 << 16) - 5, dtype=torch.float64, device="cuda")
    gP = torch.randn(1, dtype=torch.float64, device="cuda")

    def grad():
        x = x0.clone().requires_grad_(True)
        P = pycwt_amd.cwt_power_torch(x, 1.0, 1 / 8, wavelet="morlet", hop=16)[0]
        (P * gP).sum().backward()
        W = pycwt_amd.cwt_torch(x, 1.0, 1 / 8, wavelet="morlet", hop=16)[0]
        (W.real * gP).sum().backward()
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


def test_forward_and_backward_of_config2_allocate_a_fraction_of_the_matrix(hip_library):
    """torch's peak allocation across cwt_power_torch(hop=256) forward + backward at N = 2^20 x 256 scales, fp64, stays below
    one tenth of what a rows x n0 real matrix would take (215 MB): P_h, G_h, the gradient and the cotangent are all of order
    N or rows x M."""
    m = pycwt_amd.Morlet(6)
    rows, hop = 256, 256
    s0 = 2.0 / m.flambda()
    dj = np.log2(N20 / s0) / (rows - 1)
    x = torch.randn(N20, dtype=torch.float64, device="cuda", requires_grad=True)
    pycwt_amd.cwt_power_torch(x.detach(), 1.0, dj, s0, rows - 1, m, hop=hop)       # (the plan and its scratch exist)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    P, sj, _, coi = pycwt_amd.cwt_power_torch(x, 1.0, dj, s0, rows - 1, m, hop=hop)
    saved = [tuple(t.shape) for t in P.grad_fn.saved_tensors]
    P.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    matrix = 8 * rows * N20
    print("cwt_power_torch(hop=256) forward + backward of config 2: torch's peak allocation", peak, "bytes; a rows x n0 real matrix",
          matrix)
    assert P.shape == (rows, N20 // hop) and sj.size == rows and coi.shape == (N20 // hop,) and x.grad.shape == x.shape
    assert peak < matrix // 10, "peak allocation %d bytes against a tenth of the matrix, %d" % (peak, matrix // 10)
    assert saved == [(N20,)]
