"""Gradients with respect to the scales and Morlet's f0 -- cwt_adjoint_rows_scales and the `scales=` / `f0=` keywords of
cwt_torch and cwt_power_torch -- on the CPU emulation of the HIP runtime (tests/emu).

Reference, cases and bars: tests/scale_grad_common.py.  Every error of a row is relative to S_j = sum_k |summand| of that row.
fp64 at round-off: 1e-12 (measured 5.6e-14).  fp32: 8 x the 3.011e-06 that the closed form evaluated in single precision
(complex64 FFT, float32 sums) reaches over the same cases = 2.409e-05 (the code measured 7.6e-06).  fp64 at
set_tolerance(1e-9): 4 x the measured 2.170e-09, rounded up to a power of ten = 1e-8 (below 1e3 x the tolerance).
profiles/scale_grad_accuracy.txt, written by tests/perf/scale_grad_accuracy.py.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hop_common as hc
import pycwt_amd
import scale_grad_common as sc
from oracle import cwt_oracle as orc
from test_adjoint_emulated import FORMS_OPTS
from test_hop_emulated import LOCKSTEP, WAVE_SCHEDULES, launch_log, run_adjoint, schedule  # noqa: F401  (schedule: a fixture)

PRECS = [64, 32]
EINVAL = -1
ALL_CASES = sc.ABI_CASES + sc.HOP_CASES


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the C ABI against the closed form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ALL_CASES, ids=[sc.case_id(c) for c in ALL_CASES])
def test_abi_against_the_closed_form(emu_library, case, prec):
    """sgrad within the bar of the closed form (both columns; Paul's and DOG's f0 column exactly 0); in fp64 also at
    set_tolerance(1e-9) within BAR_TOL9; xbar bit-identical to cwt_adjoint_rows / cwt_adjoint_rows_hop; xbar_dev = NULL and a
    second run give the same sgrad bits."""
    logn, n0, hop, kind, param = case
    sj, x, G, ref, S = sc.case_reference(case, prec)
    with hc.Device(emu_library, 1 << logn, prec) as dev:
        got, xbar = sc.run(dev, kind, param, sj, x, G, hop)
        r = sc.ratio(got, ref, S)
        print("sgrad against the closed form:", sc.case_id(case), prec, r, "bar", sc.BAR[prec])
        assert r <= sc.BAR[prec], (r, sc.BAR[prec])
        if kind != orc.MORLET:
            assert np.all(got[:, 1] == 0)
        alone, none = sc.run(dev, kind, param, sj, x, G, hop, want_xbar=False)
        assert none is None and np.array_equal(bits(alone), bits(got))
        if hop == 1:
            dev.plan.set_option("adjoint_poly", 0)
            gd, xb = dev.up(G), dev.up(np.zeros(n0, dtype=dev.real))
            dev.plan.adjoint_rows(gd.ptr, 1, G.size, n0, n0, kind, param, 1.0, sj, xb.ptr, n0)
            want = xb.download(dev.plan, (1, n0), dev.real)
        else:
            want = run_adjoint(dev, G[None], n0, hop, kind, param, sj)
        assert np.array_equal(bits(xbar), bits(want))
        if prec == 64:
            dev.plan.set_tolerance(sc.TOL9)
            r9 = sc.ratio(sc.run(dev, kind, param, sj, x, G, hop)[0], ref, S)
            print("... at tolerance 1e-9:", r9, "bar", sc.BAR_TOL9)
            assert r9 <= sc.BAR_TOL9 <= 1e3 * sc.TOL9, (r9, sc.BAR_TOL9)


def test_the_scales_reach_both_ends_of_the_band(emu_library):
    """What the cases are chosen for: the first row's band is cut at Nyquist (DOG: two-sided through the negative bins, bin -N/2
    included), the last row has at most 4 bins, and the 2^15 case has at least three rows of more than two slices."""
    for logn in (12, 15, 16):
        N = 1 << logn
        for kind, param in sc.MOTHERS:
            sj = sc.scales(N, kind, param)
            nband = sc.band_sizes(N, kind, param, sj)
            assert nband[0] >= 0.99 * (N if kind == orc.DOG else N // 2) and 1 <= nband[-1] <= 4, (kind, param, nband)
            if kind == orc.DOG:
                bank = np.abs(orc.filter_bank(sj[:1], orc.angular_freqs(N, 1.0), N, orc.Mother(kind, param), True))
                assert bank[0, N // 2] > 1e-16 * bank.max()
    slice_len = int(re.search(r"SGRAD_SLICE\s*=\s*(\d+)", open(HEADER).read()).group(1))
    logn, _, _, kind, param = sc.ABI_CASES[-1]
    assert logn == 15 and (sc.band_sizes(1 << logn, kind, param, sc.scales(1 << logn, kind, param)) > 2 * slice_len).sum() >= 3


@pytest.mark.parametrize("prec", PRECS)
def test_xbar_with_every_row_form_in_the_table(emu_library, prec):
    """2^15 with the table holding polynomial, overlap-save and band-passed rows (FORMS_OPTS): every row takes the general path
    here, so xbar has the bits of cwt_adjoint_rows with adjoint_poly = 0, and sgrad stays within the bar."""
    N, kind, param = 1 << 15, orc.MORLET, 6
    n0 = N - 77
    sj = hc.scales(N, kind, param, 24)
    rng = np.random.default_rng(61)
    x = rng.standard_normal(n0).astype(hc.types(prec)[0])
    G = (rng.standard_normal((len(sj), n0)) + 1j * rng.standard_normal((len(sj), n0))).astype(hc.types(prec)[1])
    ref, S = sc.reference(kind, param, sj, x, G, N)
    with hc.Device(emu_library, N, prec, options=dict(FORMS_OPTS)) as dev:
        hc.run_full(dev, x, kind, param, sj)
        assert "poly" in {c.split("/")[0] for c in dev.plan.row_classes()}
        got, xbar = sc.run(dev, kind, param, sj, x, G)
        assert sc.ratio(got, ref, S) <= sc.BAR[prec]
        gd, xb = dev.up(G), dev.up(np.zeros(n0, dtype=dev.real))
        dev.plan.set_option("adjoint_poly", 0)
        dev.plan.adjoint_rows(gd.ptr, 1, G.size, n0, n0, kind, param, 1.0, sj, xb.ptr, n0)
        assert np.array_equal(bits(xbar[0]), bits(xb.download(dev.plan, (n0,), dev.real)))


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [sc.ABI_CASES[-1], (12, 4019, 16, orc.MORLET, 6)], ids=sc.case_id)
def test_batch_accumulate_and_independence_of_rows_and_chunks(emu_library, case, prec):
    """A batch of 3 equals the three single calls added in order in double (xbar: the single calls' bits); accumulate = 1 adds to
    sgrad and to xbar; a row's bits do not change when it is computed alone, or with the chunk forced to one row (option
    "chunk_rows" = 1: the chunk follows that option, not max_rows)."""
    logn, n0, hop, kind, param = case
    N = 1 << logn
    sj, X, G = sc.inputs(case, prec, nb=3)
    rows = len(sj)
    with hc.Device(emu_library, N, prec) as dev:
        whole, xbar = sc.run(dev, kind, param, sj, X, G, hop)
        singles = [sc.run(dev, kind, param, sj, X[b], G[b], hop) for b in range(3)]
        ordered = (singles[0][0] + singles[1][0]) + singles[2][0]
        assert np.array_equal(whole, ordered)
        for b in range(3):
            assert np.array_equal(bits(xbar[b]), bits(singles[b][1][0])), b
        base_s = np.random.default_rng(1).standard_normal((rows, 2))
        base_x = np.random.default_rng(2).standard_normal((3, n0)).astype(dev.real)
        acc_s, acc_x = sc.run(dev, kind, param, sj, X, G, hop, onto=base_x, sgrad_onto=base_s)
        assert np.array_equal(acc_s, base_s + whole) and np.array_equal(acc_x, base_x + xbar)
        one = singles[0][0]
        for j in (0, 2, rows - 1):
            alone, _ = sc.run(dev, kind, param, sj[j:j + 1], X[0], G[0, j:j + 1], hop)
            assert np.array_equal(bits(alone[0]), bits(one[j])), j
    with hc.Device(emu_library, N, prec, options={"chunk_rows": 1}) as dev:
        by_one, xbar_one = sc.run(dev, kind, param, sj, X[0], G[0], hop)
        assert np.array_equal(bits(by_one), bits(one))


# ---- launch logs ------------------------------------------------------------------------------------------------------------------
def test_existing_exports_launch_no_sgrad_kernel_and_refusals_launch_nothing(emu_library):
    lib = emu_library
    dll = lib.dll
    N, n0, hop = 1 << 12, 4000, 16
    nch = -(-n0 // hop)
    sj = np.ascontiguousarray(sc.scales(N, orc.MORLET, 6))
    rows = len(sj)
    sp = sj.ctypes.data_as(C.POINTER(C.c_double))
    P = C.c_void_p
    with hc.Device(lib, N, 64, max_rows=rows) as dev:
        g = dev.up(np.zeros((rows, n0), dtype=np.complex128))
        xh, xb, sg = dev.up(np.zeros(N, dtype=np.complex128)), dev.up(np.zeros(n0)), dev.up(np.zeros((rows, 2)))
        dev.plan.sync()
        dll.hipemu_clear_launched()
        dev.plan.adjoint_rows(g.ptr, 1, rows * n0, n0, n0, orc.MORLET, 6.0, 1.0, sj, xb.ptr, n0)
        dev.plan.adjoint_rows_hop(g.ptr, 1, rows * nch, nch, hop, n0, orc.MORLET, 6.0, 1.0, sj, xb.ptr, n0)
        log = launch_log(lib)
        assert log and not any("sgrad" in s for s in log), log

        def call(G=g.ptr, nbatch=1, ldg=None, nc=None, hop_=1, n0_=n0, xhat=xh.ptr, xhat_ld=N, mother=0, s=sp, xbar=xb.ptr, xbar_ld=n0,
                 out=sg.ptr, gb=None):
            nc = -(-n0_ // max(hop_, 1)) if nc is None else nc
            ldg = nc if ldg is None else ldg
            return dll.cwt_adjoint_rows_scales(dev.plan.h, P(G), nbatch, rows * ldg if gb is None else gb, ldg, nc, hop_, n0_, P(xhat), xhat_ld,
                                               mother, 6.0, 1.0, s, rows, P(xbar), xbar_ld, 0, P(out))
        dev.plan.sync()
        dll.hipemu_clear_launched()
        refused = [
            ("G NULL", call(G=None)), ("scales NULL", call(s=None)), ("xhat NULL", call(xhat=None)), ("sgrad NULL", call(out=None)),
            ("a filter bank", call(mother=3)), ("nbatch 0", call(nbatch=0)), ("ncols != n0", call(nc=n0 - 1)), ("n0 > nfft", call(n0_=N + 1)),
            ("n0 = 0", call(n0_=0, nc=0)), ("ldg < ncols", call(ldg=n0 - 1)), ("xbar_ld < n0", call(xbar_ld=n0 - 1)),
            ("g_batch_ld", call(nbatch=2, gb=rows * n0 - 1)), ("xhat_ld < nfft", call(nbatch=2, xhat_ld=N - 1)),
            ("rows > max_rows", call(nbatch=2, hop_=hop)), ("hop = 0", call(hop_=0, nc=n0)), ("hop < 0", call(hop_=-2, nc=n0)),
            ("hop not a power of two", call(hop_=12)), ("M < 16", call(hop_=512)), ("hop: ncols_h", call(hop_=hop, nc=nch - 1)),
            ("hop: ldg", call(hop_=hop, ldg=nch - 1)), ("hop: xbar_ld", call(hop_=hop, xbar_ld=n0 - 1)),
        ]
        for name, rc in refused:
            assert rc == EINVAL and lib.cwt_last_error(), name
        assert launch_log(lib) == set()
        assert call() == 0 and call(hop_=hop) == 0 and call(xbar=None) == 0            # ... and the good calls go through
        assert all(any(name in s for s in launch_log(lib)) for name in SGRAD_KERNELS)


# ---- wavefront schedules ----------------------------------------------------------------------------------------------------------
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pycwt_amd", "csrc", "cwt_kernels_sgrad.hpp")
SGRAD_KERNELS = set(re.findall(r"__global__[^{;]*?\b(sgrad_\w+)\s*\(", open(HEADER).read()))


def test_the_header_names_its_kernels_sgrad():
    text = open(HEADER).read()
    assert SGRAD_KERNELS == {"sgrad_partial", "sgrad_sum"}
    assert not re.findall(r"__global__[^{;]*?\b(k_\w+)\s*\(", text)          # (test_emu_schedules.py gates every k_* of csrc/)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [(12, 4019, 1, orc.DOG, 2), (12, 4019, 16, orc.MORLET, 6), sc.ABI_CASES[-1]], ids=sc.case_id)
def test_wavefront_schedules_give_the_bits_of_the_default_order(emu_library, schedule, case, prec):
    """Every sgrad_* kernel of the header under forward, reverse and seeded wavefront orders: the bits of the lockstep order (the
    LDS tree of sgrad_partial uses workgroup barriers only), for a batch of 2."""
    logn, n0, hop, kind, param = case
    sj, X, G = sc.inputs(case, prec, nb=2)

    def once():
        with hc.Device(emu_library, 1 << logn, prec) as dev:
            return [bits(a).copy() for a in sc.run(dev, kind, param, sj, X, G, hop)]
    schedule(LOCKSTEP)
    base = once()
    for label, k, s in WAVE_SCHEDULES:
        schedule(k, s)
        emu_library.dll.hipemu_clear_launched()
        got = once()
        log = launch_log(emu_library)
        assert all(any(name in s for s in log) for name in SGRAD_KERNELS), (label, log)
        for a, b in zip(base, got):
            assert np.array_equal(a, b), label


# ---- torch on the emulated library ------------------------------------------------------------------------------------------------
@pytest.fixture()
def fresh_engines(emulated, monkeypatch):
    from pycwt_amd import autograd
    monkeypatch.setattr(autograd, "_engines", {})
    yield autograd
    for eng in autograd._engines.values():
        eng.plan.close()


WAVELETS = {"morlet": (orc.MORLET, 6), "paul": (orc.PAUL, 4), "dog": (orc.DOG, 2)}


def torch_scales(torch, N, kind, param, rows=6):
    """scales every mother keeps at dt = 1 (Paul's NaN-row rule drops s > 709 / pi there), from the smallest to a narrow band"""
    m = orc.Mother(kind, param)
    s0, s1 = 2.0 / m.flambda(), 200.0 if kind == orc.PAUL else 0.2 * N
    return torch.tensor(s0 * (s1 / s0) ** (np.arange(rows) / (rows - 1)), dtype=torch.float64)


def test_values_with_scales_against_the_oracle(fresh_engines):
    torch = pytest.importorskip("torch")
    n0, N = 3000, 4096
    x = np.random.default_rng(71).standard_normal(n0)
    for name, (kind, param) in WAVELETS.items():
        t = torch_scales(torch, N, kind, param)
        W, sj, freqs, coi = pycwt_amd.cwt_torch(torch.as_tensor(x), 1.0, wavelet=name, scales=t)
        ref = orc.cwt_rows(x, 1.0, t.numpy(), orc.Mother(kind, param), N=N, intended=True)[:, :n0]
        assert isinstance(sj, np.ndarray) and np.array_equal(sj, t.numpy()) and isinstance(freqs, np.ndarray) and coi.shape == (n0,)
        np.testing.assert_allclose(freqs, 1 / (orc.Mother(kind, param).flambda() * sj), rtol=1e-15)
        assert np.abs(W.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
        P = pycwt_amd.cwt_power_torch(torch.as_tensor(x), 1.0, wavelet=name, scales=t)[0]
        assert np.abs(P.numpy() - np.abs(ref) ** 2).max() <= 1e-12 * (np.abs(ref) ** 2).max()


@pytest.mark.parametrize("hop", [None, 16])
@pytest.mark.parametrize("shape", [(3000,), (2, 3000)], ids=["single", "batch2"])
@pytest.mark.parametrize("name", list(WAVELETS))
def test_torch_gradients_against_the_closed_form(fresh_engines, name, shape, hop):
    """d/d scales (and d/d f0 for Morlet) of Re sum conj(C) W through cwt_torch and of sum gP P through cwt_power_torch, fp64,
    against the closed form: sgrad[:, 0] / s and sum sgrad[:, 1], summed over the batch; 1e-12 of S (the power route: G = 2 gP W of
    the oracle's W)."""
    torch = pytest.importorskip("torch")
    kind, param = WAVELETS[name]
    n0, N, h = shape[-1], 4096, hop or 1
    rng = np.random.default_rng(72)
    X = rng.standard_normal(shape)
    t0 = torch_scales(torch, N, kind, param)
    rows, nch = len(t0), -(-n0 // h)
    m = orc.Mother(kind, param)
    Wref = np.stack([orc.cwt_rows(xb, 1.0, t0.numpy(), m, N=N, intended=True)[:, :n0:h] for xb in np.atleast_2d(X)])
    Cn = rng.standard_normal(Wref.shape) + 1j * rng.standard_normal(Wref.shape)
    gPn = rng.standard_normal(Wref.shape)
    for power in (False, True):
        t = t0.clone().requires_grad_(True)
        f0 = torch.tensor(float(param), dtype=torch.float64, requires_grad=True) if kind == orc.MORLET else None
        xt = torch.as_tensor(X)
        if power:
            out = pycwt_amd.cwt_power_torch(xt, 1.0, wavelet=name, hop=hop, scales=t, f0=f0)[0]
            (out * torch.as_tensor(gPn.reshape(out.shape))).sum().backward()
            Gn = 2 * gPn * Wref
        else:
            out = pycwt_amd.cwt_torch(xt, 1.0, wavelet=name, hop=hop, scales=t, f0=f0)[0]
            (out.conj() * torch.as_tensor(Cn.reshape(out.shape))).real.sum().backward()
            Gn = Cn
        assert out.shape == tuple(shape[:-1]) + (rows, nch)
        ref, S = np.zeros((rows, 2)), np.zeros((rows, 2))
        for b, xb in enumerate(np.atleast_2d(X)):
            r, s = sc.reference(kind, param, t0.numpy(), xb, Gn[b], N, h)
            ref, S = ref + r, S + s
        assert t.grad.dtype == torch.float64 and t.grad.shape == t0.shape
        assert np.all(np.abs(t.grad.numpy() * t0.numpy() - ref[:, 0]) <= sc.BAR[64] * S[:, 0]), power
        if f0 is not None:
            assert f0.grad.shape == () and abs(float(f0.grad) - ref[:, 1].sum()) <= sc.BAR[64] * S[:, 1].sum(), power


@pytest.mark.parametrize("shape", [(60,), (2, 33)])
def test_gradcheck_with_respect_to_scales_and_f0(fresh_engines, shape):
    """The wiring (the division by s, the batch sum, the complex convention) against central differences, fp64: eps = 1e-6 and
    atol = rtol = 1e-6; the forward's round-off, 4e-15 max|W| / eps, stays below that for inputs scaled to max|W| <= 10."""
    torch = pytest.importorskip("torch")
    x = torch.as_tensor(np.random.default_rng(73).standard_normal(shape))
    t = torch.tensor([1.3, 2.9, 6.2], dtype=torch.float64, requires_grad=True)
    f0 = torch.tensor(5.5, dtype=torch.float64, requires_grad=True)
    W = pycwt_amd.cwt_torch(x, 0.5, scales=t.detach())[0]
    x = x * (5.0 / float(W.abs().max()))
    xs = x * 0.5                                                   # (|W|^2 <= 10 as well)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6)
    if len(shape) == 1:
        assert torch.autograd.gradcheck(lambda s, f: pycwt_amd.cwt_torch(x, 0.5, wavelet="morlet", scales=s, f0=f)[0], (t, f0), **kw)
        assert torch.autograd.gradcheck(lambda s: pycwt_amd.cwt_power_torch(xs, 0.5, wavelet="dog", scales=s)[0], (t,), **kw)
        assert torch.autograd.gradcheck(lambda s: pycwt_amd.cwt_torch(x, 0.5, wavelet="morlet", hop=4, scales=s)[0], (t,), **kw)
    else:
        assert torch.autograd.gradcheck(lambda s, f: pycwt_amd.cwt_power_torch(xs, 0.5, wavelet="morlet", scales=s, f0=f)[0], (t, f0), **kw)
        assert torch.autograd.gradcheck(lambda s: pycwt_amd.cwt_torch(x, 0.5, wavelet="paul", scales=s)[0], (t,), **kw)


def test_backward_without_a_scale_gradient_is_the_present_one_and_x_grad_keeps_its_bits(fresh_engines):
    """2^16 points (polynomial rows in the table).  scales= given but not requiring grad: the backward's launch log equals that
    of cwt_torch without the keyword, no sgrad kernel, the same x.grad bits.  x, scales and f0 requiring grad together: x.grad has
    the bits of the present path run with adjoint_poly = 0."""
    torch = pytest.importorskip("torch")
    lib = fresh_engines._hip.load()
    n0 = (1 << 16) - 5
    x0 = torch.as_tensor(np.random.default_rng(74).standard_normal(n0))

    def backward_log(**kw):
        x = x0.clone().requires_grad_(True)
        W, sj = pycwt_amd.cwt_torch(x, 1.0, 1 / 2, **kw)[:2] if not kw else pycwt_amd.cwt_torch(x, 1.0, **kw)[:2]
        for eng in fresh_engines._engines.values():
            eng.plan.sync()
        lib.dll.hipemu_clear_launched()
        W.abs().sum().backward()
        return launch_log(lib), x.grad.numpy().copy(), sj
    log0, g0, sj = backward_log()
    assert any("k_poly_moments" in s for s in log0)
    t = torch.tensor(sj, dtype=torch.float64)
    log1, g1, sj1 = backward_log(scales=t)
    assert np.array_equal(sj1, sj) and log1 == log0 and np.array_equal(bits(g1), bits(g0))
    log2, g2, _ = backward_log(scales=t.clone().requires_grad_(True), f0=torch.tensor(6.0, dtype=torch.float64, requires_grad=True))
    assert all(any(name in s for s in log2) for name in SGRAD_KERNELS) and not any("k_poly_moments" in s for s in log2)
    for eng in fresh_engines._engines.values():
        eng.plan.set_option("adjoint_poly", 0)
    log3, g3, _ = backward_log()
    assert not any("sgrad" in s for s in log3) and np.array_equal(bits(g2), bits(g3))
    assert len(fresh_engines._engines) == 1


def test_only_what_needs_a_gradient_is_computed(fresh_engines):
    """x without requires_grad: no accumulator, no k_adj_out; the scale gradient has the bits of the run that also asks for x.grad"""
    torch = pytest.importorskip("torch")
    lib = fresh_engines._hip.load()
    n0 = 3000
    xn = np.random.default_rng(75).standard_normal((2, n0))
    grads = []
    for need_x in (False, True):
        x = torch.as_tensor(xn).requires_grad_(need_x)
        t = torch_scales(torch, 4096, orc.DOG, 2).requires_grad_(True)
        P = pycwt_amd.cwt_power_torch(x, 1.0, wavelet="dog", scales=t)[0]
        lib.dll.hipemu_clear_launched()
        P.sum().backward()
        log = launch_log(lib)
        assert any("k_adj_out" in s for s in log) == need_x and any("k_adj_accum" in s for s in log) == need_x
        assert (x.grad is not None) == need_x
        grads.append(t.grad.numpy().copy())
    assert np.array_equal(bits(grads[0]), bits(grads[1]))


def test_refusals_of_the_keywords(fresh_engines):
    torch = pytest.importorskip("torch")
    x = torch.zeros(100, dtype=torch.float64)
    t = torch.tensor([2.0, 4.0], dtype=torch.float64)
    f0 = torch.tensor(6.0, dtype=torch.float64)
    for fn in (pycwt_amd.cwt_torch, pycwt_amd.cwt_power_torch):
        for kw in (dict(dj=1 / 4), dict(s0=2.0), dict(J=5), dict(freqs=np.array([0.1, 0.2]))):
            with pytest.raises(ValueError, match="scales= replaces"):
                fn(x, 1.0, scales=t, **kw)
        for bad in (t[None], t.float(), torch.tensor([2.0, 0.0], dtype=torch.float64), torch.tensor([2.0, -1.0], dtype=torch.float64),
                    torch.tensor([2.0, float("nan")], dtype=torch.float64), torch.tensor([2.0, float("inf")], dtype=torch.float64),
                    np.array([2.0, 4.0])):
            with pytest.raises(ValueError, match="scales must"):
                fn(x, 1.0, scales=bad)
        for wavelet in ("paul", "dog", pycwt_amd.DOG(6)):
            with pytest.raises(ValueError, match="Morlet"):
                fn(x, 1.0, wavelet=wavelet, f0=f0)
        for bad in (torch.tensor([6.0], dtype=torch.float64), torch.tensor(6.0), 6.0):
            with pytest.raises(ValueError, match="0-dim float64"):
                fn(x, 1.0, f0=bad)
        with pytest.raises(TypeError):
            fn(x, 1.0, 1 / 12, -1, -1, "morlet", None, True, None, t)             # keyword only


def test_f0_replaces_the_wavelet_objects_f0(fresh_engines):
    torch = pytest.importorskip("torch")
    x = torch.as_tensor(np.random.default_rng(76).standard_normal(500))
    t = torch.tensor([2.0, 5.0, 9.0], dtype=torch.float64)
    a = pycwt_amd.cwt_torch(x, 1.0, wavelet=pycwt_amd.Morlet(6), scales=t, f0=torch.tensor(4.5, dtype=torch.float64))
    b = pycwt_amd.cwt_torch(x, 1.0, wavelet=pycwt_amd.Morlet(4.5), scales=t)
    assert np.array_equal(bits(a[0].numpy()), bits(b[0].numpy())) and np.array_equal(a[2], b[2])


def test_scales_dropped_by_pauls_nan_row_rule_get_gradient_zero(fresh_engines):
    torch = pytest.importorskip("torch")
    n0, N = 3000, 4096
    sj = sc.scales(N, orc.PAUL, 4)
    bad = orc.dropped_rows(sj, 1.0, orc.Mother(orc.PAUL, 4))
    assert bad.any() and not bad.all()
    x = torch.as_tensor(np.random.default_rng(77).standard_normal(n0))
    t = torch.tensor(sj, dtype=torch.float64, requires_grad=True)
    W, kept, freqs, _ = pycwt_amd.cwt_torch(x, 1.0, wavelet="paul", scales=t)
    assert W.shape == ((~bad).sum(), n0) and np.array_equal(kept, sj[~bad]) and len(freqs) == len(kept)
    W.abs().pow(2).sum().backward()
    g = t.grad.numpy()
    assert np.all(g[bad] == 0) and np.all(g[~bad] != 0)
