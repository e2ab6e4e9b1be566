"""Gradients with respect to the scales and Morlet's f0 (cwt_adjoint_rows_scales, the `scales=` / `f0=` keywords) on a real
MI355X: the closed-form reference and the bars of the emulated tests (tests/scale_grad_common.py: 1e-12 of S_j in fp64,
2.409e-05 in fp32 -- 8 x what the closed form reaches in single precision) at 2^15 and at 2^18, where the bands reach 2^17
bins (2^18 for DOG) and need tens of slices; the decimated adjoint at 2^16 / 16 and 2^18 / 64; a batch; torch's gradcheck; a
second stream.  Nothing outside the repository is read."""
import numpy as np
import pytest

import hop_common as hc
import pycwt_amd
import scale_grad_common as sc
from oracle import cwt_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", sc.GPU_CASES, ids=[sc.case_id(c) for c in sc.GPU_CASES])
def test_abi_against_the_closed_form_on_the_device(hip_library, case, prec):
    """16 scales from the smallest to the largest; sgrad within the bar; xbar_dev = NULL gives the same sgrad bits; xbar has the
    bits of cwt_adjoint_rows with adjoint_poly = 0 / of cwt_adjoint_rows_hop."""
    logn, n0, hop, kind, param = case
    sj, x, G, ref, S = sc.case_reference(case, prec, sc.GPU_ROWS)
    if logn == 18 and hop == 1:
        assert (sc.band_sizes(1 << logn, kind, param, sj[:1]) > 20 * 2048).all()              # tens of slices
    with hc.Device(hip_library, 1 << logn, prec) as dev:
        got, xbar = sc.run(dev, kind, param, sj, x, G, hop)
        r = sc.ratio(got, ref, S)
        print("sgrad against the closed form on the device:", sc.case_id(case), prec, r, "bar", sc.BAR[prec])
        assert r <= sc.BAR[prec], (r, sc.BAR[prec])
        alone, _ = sc.run(dev, kind, param, sj, x, G, hop, want_xbar=False)
        assert np.array_equal(bits(alone), bits(got))
        gd, xb = dev.up(G), dev.up(np.zeros(n0, dtype=dev.real))
        if hop == 1:
            dev.plan.set_option("adjoint_poly", 0)
            dev.plan.adjoint_rows(gd.ptr, 1, G.size, n0, n0, kind, param, 1.0, sj, xb.ptr, n0)
        else:
            dev.plan.adjoint_rows_hop(gd.ptr, 1, G.size, G.shape[1], hop, n0, kind, param, 1.0, sj, xb.ptr, n0)
        assert np.array_equal(bits(xbar[0]), bits(xb.download(dev.plan, (n0,), dev.real)))


@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("case", [(15, 30000, 1, orc.DOG, 2), (16, (1 << 16) - 77, 16, orc.MORLET, 6)], ids=sc.case_id)
def test_a_batch_of_three_is_the_ordered_sum_of_single_calls(hip_library, case, prec):
    logn, n0, hop, kind, param = case
    sj, X, G = sc.inputs(case, prec, nb=3)
    with hc.Device(hip_library, 1 << logn, prec) as dev:
        whole, xbar = sc.run(dev, kind, param, sj, X, G, hop)
        singles = [sc.run(dev, kind, param, sj, X[b], G[b], hop) for b in range(3)]
        assert np.array_equal(whole, (singles[0][0] + singles[1][0]) + singles[2][0])
        for b in range(3):
            assert np.array_equal(bits(xbar[b]), bits(singles[b][1][0])), b
        again, _ = sc.run(dev, kind, param, sj, X, G, hop)
        assert np.array_equal(bits(again), bits(whole))


def test_gradcheck_on_the_device(hip_library):
    """n0 = 60, fp64, eps = 1e-6, atol = rtol = 1e-6 (inputs scaled to max|W| <= 10), with respect to scales and f0"""
    x = torch.randn(60, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(81))
    t = torch.tensor([1.3, 2.9, 6.2], dtype=torch.float64, requires_grad=True)
    f0 = torch.tensor(5.5, dtype=torch.float64, requires_grad=True)
    W = pycwt_amd.cwt_torch(x, 0.5, scales=t.detach())[0]
    x = x * (5.0 / float(W.abs().max()))
    xs = x * 0.5
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda s, f: pycwt_amd.cwt_torch(x, 0.5, wavelet="morlet", scales=s, f0=f)[0], (t, f0), **kw)
    assert torch.autograd.gradcheck(lambda s: pycwt_amd.cwt_power_torch(xs, 0.5, wavelet="dog", scales=s)[0], (t,), **kw)
    td = t.detach().to("cuda").requires_grad_(True)                  # scales on x's device: the gradient comes back there
    assert torch.autograd.gradcheck(lambda s: pycwt_amd.cwt_torch(x, 0.5, wavelet="morlet", hop=4, scales=s)[0], (td,), **kw)


def test_backward_on_another_stream_gives_the_same_bits(hip_library):
    x0 = torch.randn((2, (1 << 16) - 5), dtype=torch.float64, device="cuda")
    gP = torch.randn(1, dtype=torch.float64, device="cuda")
    s0 = torch.tensor(2.0 * 2 ** (np.arange(24) / 2), dtype=torch.float64)

    def grads():
        x = x0.clone().requires_grad_(True)
        t = s0.clone().requires_grad_(True)
        f0 = torch.tensor(6.0, dtype=torch.float64, requires_grad=True)
        P = pycwt_amd.cwt_power_torch(x, 1.0, scales=t, f0=f0)[0]
        (P * gP).sum().backward()
        W = pycwt_amd.cwt_torch(x, 1.0, hop=16, scales=t, f0=f0)[0]
        (W.real * gP).sum().backward()
        return x.grad, t.grad, f0.grad

    g0 = grads()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g1 = grads()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b in zip(g0, g1):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert g0[1].device.type == "cpu" and g0[0].device.type == "cuda"
