"""pycwt_amd.cwt_power_torch -- the differentiable scalogram |W|^2 whose backward recomputes W under the cotangent of P in the
row kernels' store (cwt_transform_weighted) and holds nothing of rows x n0 elements in between -- on the CPU emulation of the
HIP runtime (tests/emu): its values against cwt_torch squared, torch's gradcheck, its gradient against the route through
cwt_torch at a length where every row form is present, the adjoint identity against the oracle, what it refuses, and the
absence of state between calls.
"""
import numpy as np
import pytest

import pycwt_amd
from oracle import cwt_oracle as orc
from test_adjoint_emulated import BOUND, FORMS_OPTS, rel
from test_power_emulated import DuckMorlet, power_bound

torch = pytest.importorskip("torch")


@pytest.fixture()
def fresh_engines(emulated, monkeypatch):
    """cwt_torch / cwt_power_torch on the emulated library, with an engine cache of the test's own"""
    from pycwt_amd import autograd
    monkeypatch.setattr(autograd, "_engines", {})
    yield autograd
    for eng in autograd._engines.values():
        eng.plan.close()


MOTHERS = [("morlet", lambda: pycwt_amd.Morlet(6)), ("paul", lambda: pycwt_amd.Paul(4)), ("dog", lambda: pycwt_amd.DOG(2)),
           ("mexican_hat", lambda: pycwt_amd.MexicanHat())]


@pytest.mark.parametrize("n0", [1000, (1 << 15) - 77])
@pytest.mark.parametrize("name,mother", MOTHERS, ids=[m[0] for m in MOTHERS])
def test_values_are_cwt_torch_squared(fresh_engines, name, mother, n0):
    """A signal and a batch of 3: P against |W|^2 of cwt_torch under the rule of power_bound; sj, freqs, coi equal."""
    rng = np.random.default_rng(31)
    for shape in ((n0,), (3, n0)):
        x = torch.as_tensor(rng.standard_normal(shape))
        P, sj, freqs, coi = pycwt_amd.cwt_power_torch(x, 0.5, 1 / 4, wavelet=mother())
        W, sj_w, freqs_w, coi_w = pycwt_amd.cwt_torch(x, 0.5, 1 / 4, wavelet=mother())
        assert P.dtype == torch.float64 and P.shape == W.shape and P.device == x.device
        power_bound(P.numpy(), W.numpy(), 64)
        for a, b in ((sj, sj_w), (freqs, freqs_w), (coi, coi_w)):
            assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype


def test_values_float32(fresh_engines):
    x = torch.as_tensor(np.random.default_rng(32).standard_normal((3, 1000)), dtype=torch.float32)
    P = pycwt_amd.cwt_power_torch(x, 0.5, 1 / 4, wavelet="dog")[0]
    W = pycwt_amd.cwt_torch(x, 0.5, 1 / 4, wavelet="dog")[0]
    assert P.dtype == torch.float32
    power_bound(P.numpy(), W.numpy(), 32)


@pytest.mark.parametrize("shape", [(48,), (2, 40)])
def test_gradcheck_through_cwt_power_torch(fresh_engines, shape):
    x = torch.randn(shape, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_power_torch(t, 0.5, 1.0, wavelet="morlet")[0], (x,), atol=1e-8)


@pytest.mark.parametrize("prec", [64, 32])
def test_gradient_against_the_route_through_cwt_torch(fresh_engines, prec):
    """N = 2^15 with FORMS_OPTS: polynomial, overlap-save, band-passed and band-limited rows in one table.  Under a random
    cotangent gP the two routes hand the same adjoint G = 2 gP W up to the rounding of G (torch forms 2 gP |W| W / |W|, the row
    kernels (2 gP) W), so they agree as cwt_torch's gradient agrees with a NumPy adjoint: BOUND of test_adjoint_emulated."""
    autograd = fresh_engines
    real_t = torch.float64 if prec == 64 else torch.float32
    N, n0 = 1 << 15, (1 << 15) - 77
    m = pycwt_amd.Morlet(6)
    rng = np.random.default_rng(33)
    x0 = torch.as_tensor(rng.standard_normal(n0), dtype=real_t)
    eng = autograd._engine(torch, N, prec, 64, x0.device, pycwt_amd._hip.load())
    for k, v in FORMS_OPTS.items():
        eng.plan.set_option(k, v)

    xa = x0.clone().requires_grad_(True)
    W = pycwt_amd.cwt_torch(xa, 1.0, 1 / 4, wavelet=m)[0]
    kinds = {c.split("/")[0] for c in eng.plan.row_classes()}
    assert {"poly", "ols", "aols"} <= kinds and {"narrow", "two_pass", "narrow_k2048"} & kinds, kinds
    gP = torch.as_tensor(rng.standard_normal(tuple(W.shape)), dtype=real_t)
    (W.abs().pow(2) * gP).sum().backward()

    xb = x0.clone().requires_grad_(True)
    P = pycwt_amd.cwt_power_torch(xb, 1.0, 1 / 4, wavelet=m)[0]
    assert {c.split("/")[0] for c in eng.plan.row_classes()} == kinds and len(autograd._engines) == 1
    (P * gP).sum().backward()
    err = rel(xb.grad.numpy().astype(np.float64), xa.grad.numpy().astype(np.float64))
    print("gradient of cwt_power_torch against the route through cwt_torch, precision", prec, ":", err)
    assert xb.grad.dtype == real_t and err <= BOUND[prec], err


@pytest.mark.parametrize("wavelet,kind,param", [("morlet", orc.MORLET, 6), ("paul", orc.PAUL, 4), ("dog", orc.DOG, 2)])
def test_adjoint_identity_against_the_oracle(fresh_engines, wavelet, kind, param):
    """<xbar, v> = sum gP 2 Re(conj(W) A v) for a random real v, with W = A x and A v from the oracle: 1e-9 relative to
    |2 gP W| |A v|, the scale of the inner product (as the adjoint identity of test_adjoint_emulated is scaled)."""
    n0, N = 1000, 1024
    rng = np.random.default_rng(34)
    x = torch.as_tensor(rng.standard_normal(n0)).requires_grad_(True)
    P, sj, _, _ = pycwt_amd.cwt_power_torch(x, 1.0, 1 / 4, wavelet=wavelet)
    gP = rng.standard_normal(tuple(P.shape))
    (P * torch.as_tensor(gP)).sum().backward()
    v = rng.standard_normal(n0)
    m = orc.Mother(kind, param)
    W = orc.cwt_rows(x.detach().numpy(), 1.0, sj, m, N=N, intended=True)[:, :n0]
    Av = orc.cwt_rows(v, 1.0, sj, m, N=N, intended=True)[:, :n0]
    lhs = float(np.dot(x.grad.numpy(), v))
    rhs = float((gP * 2 * np.real(np.conj(W) * Av)).sum())
    assert abs(lhs - rhs) <= 1e-9 * np.linalg.norm(2 * gP * W) * np.linalg.norm(Av), (lhs, rhs)


def test_refuses_what_cwt_torch_refuses(fresh_engines):
    with pytest.raises(ValueError, match="pad"):
        pycwt_amd.cwt_power_torch(torch.randn(64, dtype=torch.float64), 1.0, pad=False)
    with pytest.raises(TypeError, match="float"):
        pycwt_amd.cwt_power_torch(torch.arange(64), 1.0)
    with pytest.raises(ValueError, match="built-in"):
        pycwt_amd.cwt_power_torch(torch.randn(64, dtype=torch.float64), 1.0, wavelet=DuckMorlet())
    with pytest.raises(ValueError, match="shape"):
        pycwt_amd.cwt_power_torch(torch.randn(2, 3, 64, dtype=torch.float64), 1.0)


def test_backward_saves_the_signal_only(fresh_engines):
    """What autograd holds between forward and backward: x, nothing of rows x n0 elements."""
    x = torch.randn(3000, dtype=torch.float64, requires_grad=True)
    P = pycwt_amd.cwt_power_torch(x, 1.0, 1 / 4)[0]
    saved = P.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].shape == x.shape
    P.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape


def test_no_state_leaks_into_the_other_outputs(fresh_engines):
    """cwt, cwt_power and cwt_torch give the bits they gave before a cwt_power_torch forward + backward"""
    n0 = (1 << 16) - 5
    xn = np.random.default_rng(35).standard_normal(n0)
    xt = torch.as_tensor(xn)

    def all_three():
        return (pycwt_amd.cwt(xn, 1.0, 1 / 2)[0], pycwt_amd.cwt_power(xn, 1.0, 1 / 2)[0],
                pycwt_amd.cwt_torch(xt, 1.0, 1 / 2)[0].numpy().copy())
    before = all_three()
    x = xt.clone().requires_grad_(True)
    pycwt_amd.cwt_power_torch(x, 1.0, 1 / 2)[0].sum().backward()
    after = all_three()
    assert len(fresh_engines._engines) == 1
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
