"""The adjoint of the row transform (cwt_adjoint_rows, Plan.adjoint_rows, pycwt_amd.cwt_torch) on the CPU emulation of the HIP
runtime (tests/emu):

    xbar = Re A^H G,   A: x -> W (zero padding to nfft, the rows of the scale grid, the trim to n0 columns),

against the dense operator built column by column from the oracle, against an FFT-based NumPy adjoint at lengths where every row
form is present, through the adjoint identity Re <G, A x> = <A^H G, x>, and through torch's autograd (gradcheck).
"""
import numpy as np
import pytest

from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_kernels_emulated import grid

BOUND = {64: 1e-12, 32: 1e-5}


def adjoint(lib, N, prec, kind, param, sj, G, opts=None, tol=0.0, accumulate_onto=None, forward_x=None, plan=None):
    """xbar (nbatch x n0) of G (nbatch x rows x n0) through cwt_adjoint_rows; forward_x: also the forward W of that signal first
    (the call a training step makes before its backward).  Returns (xbar, W or None, row classes of the table)."""
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    G = np.asarray(G)
    nb, rows, n0 = G.shape
    own = plan is None
    if own:
        plan = _hip.Plan(N, prec, max_rows=rows, lib=lib, options=opts)
        if tol:
            plan.set_tolerance(tol)
    es = np.dtype(real).itemsize
    Gd = _hip.DeviceBuffer(G.size * 2 * es, lib=lib)
    xb = _hip.DeviceBuffer(nb * n0 * es, lib=lib)
    Gd.upload(plan, G.astype(cplx))
    if accumulate_onto is not None:
        xb.upload(plan, np.asarray(accumulate_onto, dtype=real))
    W = None
    if forward_x is not None:
        xd, Wd = _hip.DeviceBuffer(n0 * es, lib=lib), _hip.DeviceBuffer(rows * n0 * 2 * es, lib=lib)
        xd.upload(plan, np.asarray(forward_x, dtype=real))
        plan.transform(xd.ptr, n0, kind, param, 1.0, sj, None, Wd.ptr, n0, n0)
        W = Wd.download(plan, (rows, n0), cplx)
        xd.free(); Wd.free()
    plan.adjoint_rows(Gd.ptr, nb, rows * n0, n0, n0, kind, param, 1.0, sj, xb.ptr, n0, accumulate_onto is not None)
    out = xb.download(plan, (nb, n0), real)
    classes = plan.classify(kind, param, 1.0, sj, n0, True)
    Gd.free(); xb.free()
    if own:
        plan.close()
    return out, W, classes


def dense_operator(n0, N, sj, m):
    """A (rows * n0 x n0): column i = the oracle's rows of the unit vector e_i, trimmed to n0."""
    A = np.empty((len(sj), n0, n0), dtype=np.complex128)
    for i in range(n0):
        e = np.zeros(n0)
        e[i] = 1.0
        A[:, :, i] = orc.cwt_rows(e, 1.0, sj, m, N=N, intended=True)[:, :n0]
    return A.reshape(len(sj) * n0, n0)


def numpy_adjoint(G, sj, m, N):
    """Re A^H G by FFTs: xbar = Re (1/N) DFT^H( sum_j conj(F_j) DFT(pad G_j) ), trimmed to n0."""
    rows, n0 = G.shape
    bank = orc.filter_bank(np.asarray(sj, dtype=float), orc.angular_freqs(N, 1.0), N, m, True)
    Gh = np.fft.fft(G, n=N, axis=1)
    acc = (np.conj(bank) * Gh).sum(axis=0)
    return np.real(np.fft.ifft(acc))[:n0]


def rel(a, b):
    return np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))


def random_g(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("kind,param", [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2), (orc.DOG, 3)])
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("N,n0,opts", [(256, 256, None), (256, 201, None), (128, 77, None), (256, 230, {"lmax": 16})])
def test_against_the_dense_operator(emu_library, kind, param, prec, N, n0, opts):
    """xbar = Re(A^H G) with A built column by column from the oracle: every mother, both precisions, n0 < N, and (lmax = 16)
    the two-pass transforms of the general path."""
    m = orc.Mother(kind, param)
    sj = grid(n0, 1.0, m, 24)
    A = dense_operator(n0, N, sj, m)
    G = random_g(np.random.default_rng(7), 1, len(sj), n0)
    ref = np.real(A.conj().T @ G.reshape(-1))
    xbar, _, _ = adjoint(emu_library, N, prec, kind, param, sj, G, opts)
    assert rel(xbar[0], ref) <= BOUND[prec], rel(xbar[0], ref)


FORMS_OPTS = {"poly_min_logn": 14, "ols_min_logn": 15, "aols_min_rows": 1}


def forms_case(kind, param, logn, rows, seed=3):
    N = 1 << logn
    n0 = N - 77
    m = orc.Mother(kind, param)
    sj = grid(n0, 1.0, m, rows)
    rng = np.random.default_rng(seed)
    return N, n0, m, sj, rng


@pytest.mark.parametrize("kind,param,logn", [(orc.MORLET, 6, 15), (orc.PAUL, 4, 15), (orc.DOG, 2, 15)])
def test_every_row_form_against_a_numpy_adjoint(emu_library, kind, param, logn):
    """At 2^15 with the thresholds of the fast forms lowered the table holds polynomial, overlap-save, band-passed and
    two-pass / narrow rows; the adjoint takes its own paths through them.  Round-off: as the dense test.  1e-9: the adjoint
    identity Re <G, A x> = <xbar, x> with the forward W of the same plan holds to 1e-8."""
    N, n0, m, sj, rng = forms_case(kind, param, logn, 56)
    G = random_g(rng, 1, len(sj), n0)
    x = rng.standard_normal(n0)
    xbar, W, classes = adjoint(emu_library, N, 64, kind, param, sj, G, FORMS_OPTS, forward_x=x)
    kinds = {c.split("/")[0] for c in classes}
    assert {"narrow", "two_pass", "narrow_k2048"} & kinds, classes
    if kind != orc.PAUL:                              # (Paul's rows are all too wide for the polynomial form: B > N / 64)
        assert "poly" in kinds, classes
    if kind == orc.MORLET:                            # (fp64 Paul takes the band-passed form only at a looser target)
        assert "ols" in kinds and "aols" in kinds, classes
    ref = numpy_adjoint(G[0], sj, m, N)
    assert rel(xbar[0], ref) <= BOUND[64], rel(xbar[0], ref)
    xbar9, W9, _ = adjoint(emu_library, N, 64, kind, param, sj, G, FORMS_OPTS, tol=1e-9, forward_x=x)
    lhs = np.real(np.vdot(G[0], W9))
    rhs = float(np.dot(x, xbar9[0]))
    assert abs(lhs - rhs) <= 1e-8 * np.linalg.norm(G) * np.linalg.norm(W9), (lhs, rhs)
    assert rel(xbar9[0], ref) <= 1e-8, rel(xbar9[0], ref)


@pytest.mark.parametrize("kind,param,prec,tol", [(orc.MORLET, 6, 64, 0.0), (orc.MORLET, 6, 64, 1e-9), (orc.DOG, 6, 64, 1e-9),
                                                  (orc.DOG, 2, 32, 0.0)])
def test_polynomial_transpose_agrees_with_the_general_path(emu_library, kind, param, prec, tol):
    """adjoint_poly = 0 (every row through the N-point transforms) and the default (polynomial rows through the transpose of
    their form) agree to the accuracy target."""
    N, n0, m, sj, rng = forms_case(kind, param, 15, 40)
    G = random_g(rng, 1, len(sj), n0)
    opts = dict(FORMS_OPTS)
    fast, _, classes = adjoint(emu_library, N, prec, kind, param, sj, G, opts, tol=tol)
    assert any(c.startswith("poly") for c in classes), classes
    opts["adjoint_poly"] = 0
    general, _, _ = adjoint(emu_library, N, prec, kind, param, sj, G, opts, tol=tol)
    assert not np.array_equal(fast, general)          # the two paths really differ
    bound = max(tol * 10, BOUND[prec])
    assert rel(fast, general) <= bound, rel(fast, general)


def test_batches_accumulation_and_determinism(emu_library):
    """A batch of 3 is bit-identical to 3 single calls; accumulate = 1 adds to xbar; two identical calls give the same bits."""
    N, n0, m, sj, rng = forms_case(orc.MORLET, 6, 14, 32)
    G = random_g(rng, 3, len(sj), n0)
    plan = _hip.Plan(N, 64, max_rows=len(sj), lib=emu_library, options=FORMS_OPTS)
    batch, _, _ = adjoint(emu_library, N, 64, orc.MORLET, 6, sj, G, plan=plan)
    singles = np.stack([adjoint(emu_library, N, 64, orc.MORLET, 6, sj, G[b:b + 1], plan=plan)[0][0] for b in range(3)])
    assert np.array_equal(batch, singles)
    again, _, _ = adjoint(emu_library, N, 64, orc.MORLET, 6, sj, G, plan=plan)
    assert np.array_equal(batch, again)
    base = rng.standard_normal((3, n0))
    summed, _, _ = adjoint(emu_library, N, 64, orc.MORLET, 6, sj, G, plan=plan, accumulate_onto=base)
    np.testing.assert_allclose(summed, base + batch, rtol=0, atol=1e-13 * np.abs(batch).max())
    plan.close()


def test_refuses_what_it_does_not_handle(emu_library):
    plan = _hip.Plan(256, 64, max_rows=8, lib=emu_library)
    sj = np.array([2.0, 4.0])
    buf = _hip.DeviceBuffer(2 * 256 * 16, lib=emu_library)
    with pytest.raises(_hip.HipError, match="built-in mother"):
        plan.adjoint_rows(buf.ptr, 1, 512, 256, 256, 3, 0.0, 1.0, sj, buf.ptr, 256)
    with pytest.raises(_hip.HipError, match="ncols"):
        plan.adjoint_rows(buf.ptr, 1, 512, 256, 512, orc.MORLET, 6.0, 1.0, sj, buf.ptr, 256)
    buf.free()
    plan.close()


# ---- torch ----------------------------------------------------------------------------------------------------------------

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("shape", [(60,), (2, 33)])
def test_gradcheck_through_cwt_torch(emulated, shape):
    """torch.autograd.gradcheck of cwt_torch on CPU fp64 tensors (the emulated library): a single signal and a batch."""
    import pycwt_amd
    x = torch.randn(shape, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.cwt_torch(t, 0.5, 1 / 2, wavelet="morlet")[0], (x,), atol=1e-8)


@pytest.mark.parametrize("wavelet", ["morlet", "paul", "dog"])
def test_cwt_torch_matches_cwt_and_its_gradient_is_the_adjoint(emulated, wavelet):
    """W, sj, freqs, coi as pycwt_amd.cwt returns them (Paul's NaN-row rule included); grad of sum |W|^2 = 2 Re(A^H W)."""
    import pycwt_amd
    n0 = 300
    x = torch.randn(n0, dtype=torch.float64, requires_grad=True)
    W, sj, freqs, coi = pycwt_amd.cwt_torch(x, 0.25, 1 / 8, wavelet=wavelet)
    ref = pycwt_amd.cwt(x.detach().numpy(), 0.25, 1 / 8, wavelet=wavelet)
    assert W.dtype == torch.complex128 and W.shape == ref[0].shape
    np.testing.assert_allclose(W.detach().numpy(), ref[0], rtol=0, atol=1e-12 * np.abs(ref[0]).max())
    for a, b in zip((sj, freqs, coi), ref[1:4]):
        np.testing.assert_array_equal(a, b)
    (W.abs() ** 2).sum().backward()
    m = orc.mother_from_name(wavelet)
    A = dense_operator(n0, 512, sj / 0.25, m)         # (dt = 0.25: the same filters as scales sj / dt at dt = 1)
    expect = 2 * np.real(A.conj().T @ W.detach().numpy().reshape(-1))
    assert rel(x.grad.numpy(), expect) <= 1e-12


def test_cwt_torch_refuses_what_it_does_not_handle(emulated):
    import pycwt_amd
    with pytest.raises(ValueError, match="pad"):
        pycwt_amd.cwt_torch(torch.randn(64, dtype=torch.float64), 1.0, pad=False)
    with pytest.raises(TypeError, match="float"):
        pycwt_amd.cwt_torch(torch.arange(64), 1.0)
    with pytest.raises(ValueError, match="built-in"):
        pycwt_amd.cwt_torch(torch.randn(64, dtype=torch.float64), 1.0, wavelet=object())
