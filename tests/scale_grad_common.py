"""Shared by tests/test_scale_grad_emulated.py, tests/test_scale_grad_gpu.py and tests/perf/scale_grad_accuracy.py: the cases of
cwt_adjoint_rows_scales, their closed-form reference and the bars.

Reference (NumPy complex128, the sums per row in longdouble).  With F = oracle.filter_bank(..., intended=True), f = s_j w_k,
Ghat = np.fft.fft(G placed on columns ::hop of a zero matrix, n=N) and xhat = np.fft.fft(x, n=N),

    summand_q[j, k] = Re( q(f) F[j, k] / N  conj(Ghat[j, k])  xhat[k] ),     dL/d ln s_j = sum_k summand_q[j, k]
    summand_r[j, k] = Re( r(f) F[j, k] / N  conj(Ghat[j, k])  xhat[k] ),     row j's share of dL/d f0 = sum_k summand_r[j, k]

    mother       q(f)                  r(f)
    Morlet(f0)   1/2 - f (f - f0)      f - f0
    Paul(m)      1/2 + m - f           0
    DOG(m)       1/2 + m - f^2         0

Every error of row j is judged against S_j = sum_k |summand[j, k]| (the sums cancel): |err_j| <= bar * S_j.

Bars.  fp64 at the round-off tolerance: 1e-12, the bar of the adjoint tests against the dense operator.  fp32: the same closed
form evaluated in single precision (complex64 FFT, float32 products and sums: `reference32`) has a worst |err_j| / S_j over the
cases of the emulated ABI tests, MEASURED_REF32; the bar is 8 x that (the order of summation and the FFT differ from
pocketfft's), capped at 1e-4.  fp64 at set_tolerance(1e-9): the worst ratio of the code over the same cases is MEASURED_TOL9;
the bar is 4 x that rounded up to a power of ten.  Both are written to profiles/scale_grad_accuracy.txt by
tests/perf/scale_grad_accuracy.py on the CPU emulation.
"""
import functools
import math

import numpy as np

import hop_common as hc
from oracle import cwt_oracle as orc

MOTHERS = [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2), (orc.DOG, 6)]
ROWS = 8
TOL9 = 1e-9

# profiles/scale_grad_accuracy.txt (tests/perf/scale_grad_accuracy.py, CPU emulation)
MEASURED_REF32 = 3.011e-06     # worst |reference32 - reference| / S over ABI_CASES + HOP_CASES
MEASURED_TOL9 = 2.170e-09      # worst |code at tolerance 1e-9 - reference| / S over the same cases, fp64


def pow10_ceil(v):
    return 10.0 ** math.ceil(math.log10(v))


BAR = {64: 1e-12, 32: min(8 * MEASURED_REF32, 1e-4)}
BAR_TOL9 = pow10_ceil(4 * MEASURED_TOL9)

# (log2 nfft, n0, hop, kind, param): the emulated ABI cases ...
ABI_CASES = [(12, n0, 1, kind, param) for n0 in (3000, 1 << 12) for kind, param in MOTHERS] + [(15, (1 << 15) - 77, 1, orc.DOG, 2)]
# ... the decimated ones: the (log2 nfft, hop) pairs of hop_common
HOP_CASES = [(logn, (1 << logn) - 77, hop, kind, param) for logn, hop in hc.SHAPES for kind, param in MOTHERS]
# ... and those of the GPU tests
GPU_MOTHERS = [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2)]
GPU_CASES = ([(15, 30000, 1, kind, param) for kind, param in GPU_MOTHERS] + [(18, 1 << 18, 1, kind, param) for kind, param in GPU_MOTHERS]
             + [(16, (1 << 16) - 77, 16, orc.MORLET, 6), (18, (1 << 18) - 77, 64, orc.DOG, 2)])
GPU_ROWS = 16


def case_id(c):
    return "2^%d-n0_%d-hop%d-%s%g" % (c[0], c[1], c[2], ["morlet", "paul", "dog"][c[3]], c[4])


def scales(N, kind, param, rows=ROWS):
    """`rows` scales, log-spaced from the smallest the grid allows (Fourier period 2 dt, dt = 1: the band is cut at Nyquist; DOG's
    is two-sided, wraps through the negative bins and includes bin -N / 2) to one whose band has at most 4 bins (s = N; Paul,
    whose profile f^m e^-f reaches f ~ 50 at round-off, 2.5 N)."""
    m = orc.Mother(kind, param)
    s0, s1 = 2.0 / m.flambda(), (2.5 if kind == orc.PAUL else 1.0) * N
    return s0 * (s1 / s0) ** (np.arange(rows) / (rows - 1))


def band_sizes(N, kind, param, sj, floor=1e-16):
    """bins of each row whose filter is above `floor` of its peak (what the row table keeps at round-off in fp64)"""
    bank = np.abs(orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, orc.Mother(kind, param), True))
    return (bank > floor * bank.max(axis=1, keepdims=True)).sum(axis=1)


def inputs(case, prec, nb=1, rows=ROWS, seed=5):
    """(sj, x: nb x n0 reals, G: nb x rows x ncols complex) of a case, seeded, rounded to the precision under test"""
    logn, n0, hop, kind, param = case
    real, cplx = hc.types(prec)
    rng = np.random.default_rng(seed + 1000 * logn + hop + 7 * kind + int(param))
    sj = scales(1 << logn, kind, param, rows)
    nch = -(-n0 // hop)
    x = rng.standard_normal((nb, n0)).astype(real)
    G = (rng.standard_normal((nb, rows, nch)) + 1j * rng.standard_normal((nb, rows, nch))).astype(cplx)
    return sj, x, G


def qr(kind, param, f):
    if kind == orc.MORLET:
        return 0.5 - f * (f - param), f - param
    if kind == orc.PAUL:
        return 0.5 + param - f, np.zeros_like(f)
    return 0.5 + param - f * f, np.zeros_like(f)


def reference(kind, param, sj, x, G, N, hop=1, dt=1.0):
    """(sgrad: rows x 2 float64, S: rows x 2) for one signal x (n0,) and its cotangent G (rows x ceil(n0 / hop))"""
    x = np.asarray(x, dtype=np.float64)
    n0 = x.size
    sj = np.asarray(sj, dtype=np.float64)
    full = np.zeros((len(sj), n0), dtype=np.complex128)
    full[:, ::hop] = np.asarray(G).astype(np.complex128)
    w = orc.angular_freqs(N, dt)
    bank = orc.filter_bank(sj, w, N, orc.Mother(kind, param), True)
    term = bank / N * np.conj(np.fft.fft(full, n=N, axis=1)) * np.fft.fft(x, n=N)[None, :]
    q, r = qr(kind, param, sj[:, None] * w[None, :])
    out, S = np.empty((len(sj), 2)), np.empty((len(sj), 2))
    for c, poly in enumerate((q, r)):
        summand = (poly * term).real.astype(np.longdouble)
        out[:, c] = summand.sum(axis=1).astype(np.float64)
        S[:, c] = np.abs(summand).sum(axis=1).astype(np.float64)
    return out, S


def reference32(kind, param, sj, x, G, N, hop=1, dt=1.0):
    """the same closed form in single precision: complex64 FFTs (scipy.fft keeps the precision of its input), float32 sums"""
    import scipy.fft as sfft
    x = np.asarray(x, dtype=np.float32)
    n0 = x.size
    sj = np.asarray(sj, dtype=np.float64)
    full = np.zeros((len(sj), n0), dtype=np.complex64)
    full[:, ::hop] = np.asarray(G).astype(np.complex64)
    w = orc.angular_freqs(N, dt)
    bank = (orc.filter_bank(sj, w, N, orc.Mother(kind, param), True) / N).astype(np.complex64)
    gh, xh = sfft.fft(full, n=N, axis=1), sfft.fft(x, n=N)
    assert gh.dtype == np.complex64 and xh.dtype == np.complex64
    term = bank * np.conj(gh) * xh[None, :]
    f = (sj[:, None] * w[None, :]).astype(np.float32)
    q, r = qr(kind, np.float32(param), f)
    out = np.empty((len(sj), 2), dtype=np.float32)
    for c, poly in enumerate((q, r)):
        out[:, c] = (poly.astype(np.float32) * term.real).sum(axis=1, dtype=np.float32)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(case, prec, rows=ROWS):
    """(sj, x (n0,), G (rows x ncols), sgrad, S) of a case: computed once, read-only, shared by the tests"""
    sj, x, G = inputs(case, prec, 1, rows)
    ref, S = reference(case[3], case[4], sj, x[0], G[0], 1 << case[0], case[2])
    for a in (sj, x, G, ref, S):
        a.flags.writeable = False
    return sj, x[0], G[0], ref, S


def ratio(got, ref, S):
    """worst |err_j| / S_j over rows and both columns (a column whose S is 0 everywhere -- r of Paul and DOG -- must be 0)"""
    got, err = np.asarray(got, dtype=np.float64), np.abs(np.asarray(got, dtype=np.float64) - ref)
    zero = S == 0
    assert np.all(got[zero] == 0), got[zero]
    return float((err[~zero] / S[~zero]).max()) if (~zero).any() else 0.0


def run(dev, kind, param, sj, x, G, hop=1, want_xbar=True, onto=None, sgrad_onto=None, dt=1.0):
    """cwt_adjoint_rows_scales of x ((n0,) or (nb, n0)) and G ((rows, ncols) or (nb, rows, ncols)) on `dev` (hop_common.Device):
    (sgrad rows x 2 float64, xbar nb x n0 or None).  onto / sgrad_onto: accumulate = 1 onto these."""
    x = np.atleast_2d(np.asarray(x, dtype=dev.real))
    G = np.asarray(G, dtype=dev.cplx)
    G = G[None] if G.ndim == 2 else G
    nb, n0 = x.shape
    rows, nch = G.shape[1:]
    N = dev.plan.nfft
    xd, gd, xh = dev.up(x), dev.up(G), dev.up(np.zeros((nb, N), dtype=dev.cplx))
    dev.plan.fft_rows(xd.ptr, False, nb, n0, n0, xh.ptr)
    acc = onto is not None or sgrad_onto is not None
    fill = 0.0 if acc else np.nan
    sg = dev.up(np.full((rows, 2), fill) if sgrad_onto is None else np.asarray(sgrad_onto, dtype=np.float64))
    xb = None
    if want_xbar:
        xb = dev.up(np.full((nb, n0), fill, dtype=dev.real) if onto is None else np.asarray(onto, dtype=dev.real))
    dev.plan.adjoint_rows_scales(gd.ptr, nb, rows * nch, nch, hop, n0, xh.ptr, N, kind, param, dt, sj, xb.ptr if xb else None, n0, sg.ptr,
                                 acc)
    return sg.download(dev.plan, (rows, 2), np.float64), xb.download(dev.plan, (nb, n0), dev.real) if xb else None
