"""Shared by tests/test_hop_emulated.py, tests/test_hop_gpu.py and tests/perf/hop_accuracy.py: the cases of the decimated
transform (cwt_transform_hop), their oracle references -- computed once per (length, signal length, mother, precision) and
shared -- and the bounds, which are MEASURED, not chosen (profiles/hop_accuracy.txt, written by tests/perf/hop_accuracy.py):

  per row, max|W_h - oracle[:, ::hop]| / max|oracle row|  <=  4 x the largest such error of the EXISTING cwt_transform at
  round-off against the same oracle on the same inputs, per precision.  The existing transform measured 4.038e-15 (fp64) and
  8.556e-06 (fp32) over the cases below; the hop rows measured 4.162e-15 and 8.757e-06.  The factor 4 is there because the
  fold adds a sum of up to hop terms in working precision before the transform.
"""
import functools

import numpy as np

from oracle import cwt_oracle as orc
from pycwt_amd import _hip

# (log2 nfft, hop): M = 2048, 256, 16 at 2^12 and M = 4096 at 2^16
SHAPES = [(12, 2), (12, 16), (12, 256), (16, 16)]
MOTHERS = [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2), (orc.DOG, 6)]
ROWS = 12
# largest per-row error of the existing cwt_transform at round-off over CASES (profiles/hop_accuracy.txt) ...
EXISTING_ERROR = {64: 4.038e-15, 32: 8.556e-06}
# ... and what a hop row may have
HOP_BOUND = {p: 4 * e for p, e in EXISTING_ERROR.items()}
# the gradient through the existing cwt_torch of a loss on W[:, ::h], against the float64 NumPy adjoint (rel. L2; same file)
EXISTING_GRAD_ERROR = {64: 8.665e-16, 32: 4.026e-07}
GRAD_BOUND = {p: 4 * e for p, e in EXISTING_GRAD_ERROR.items()}


def power_slice_bound(prec):
    """cwt_power(hop=h) against cwt_power[:, ::h], per row relative to the row's largest power.  Both are squares of a W within
    its measured error of the oracle -- e_h = HOP_BOUND, e = EXISTING_ERROR, relative to the row's peak |W| -- and
    d|W|^2 = 2 |W| d|W| <= 2 peak^2 e to first order, so the two powers differ by at most 2 e_h + 2 e of the peak power, plus
    the 4 eps of rounding that each square is allowed (tests/test_hop_emulated.py)."""
    return 2 * HOP_BOUND[prec] + 2 * EXISTING_ERROR[prec] + 8 * float(np.finfo(types(prec)[0]).eps)


def identity_bound(adjoint_bound, prec):
    """|Re <G, A_h x> - <x, A_h^H G>| relative to max(|G| |A_h x|, |x| |xbar|): each side is off by at most its operand's relative
    L2 error times that scale (Cauchy-Schwarz), and both errors are within the relative-L2 bound of the adjoint tests
    (tests/test_adjoint_emulated.BOUND: 1e-12 / 1e-5; the forward's relative L2 error is below its per-row HOP_BOUND)."""
    return 2 * adjoint_bound[prec]


def n0_of(N):
    """n0 = nfft; nfft - 77 (ncols_h * hop > n0: the last kept column is the only one of its hop); just above nfft / 2"""
    return [N, N - 77, N // 2 + 3]


CASES = [(logn, hop, n0, kind, param) for logn, hop in SHAPES for n0 in n0_of(1 << logn) for kind, param in MOTHERS]


def case_id(c):
    return "2^%d-hop%d-n0_%d-%s%g" % (c[0], c[1], c[2], ["morlet", "paul", "dog"][c[3]], c[4])


def types(prec):
    return (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)


def scales(N, kind, param, rows=ROWS):
    """from the Fourier period 2 dt (rows clipped at Nyquist: a band of about N / 2 bins, hop aliases per folded bin) to the period
    N dt (a band of a few bins: one term per folded bin), dt = 1; Paul's rows that the reference turns into NaN dropped"""
    m = orc.Mother(kind, param)
    s0 = 2.0 / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))
    return sj[~orc.dropped_rows(sj, 1.0, m)]


def signal(n0, prec, seed=3):
    """seeded white noise, rounded to the precision under test (the oracle sees the same numbers)"""
    return np.random.default_rng(seed).standard_normal(n0).astype(types(prec)[0])


@functools.lru_cache(maxsize=None)
def reference(logn, n0, kind, param, prec):
    """(sj, oracle W of the case's signal: rows x n0 complex128, its per-row peak); read-only, shared by the tests"""
    N = 1 << logn
    sj = scales(N, kind, param)
    W = orc.cwt_rows(signal(n0, prec).astype(np.float64), 1.0, sj, orc.Mother(kind, param), N=N)[:, :n0]
    W.flags.writeable = False
    return sj, W, np.abs(W).max(axis=1)


def row_error(got, ref, peak):
    return (np.abs(np.asarray(got).astype(np.complex128) - ref).max(axis=1) / peak).max()


class Device:
    """a plan and the device buffers of one test, freed together"""

    def __init__(self, lib, N, prec, max_rows=64, options=None):
        self.lib, self.prec = lib, prec
        self.real, self.cplx = types(prec)
        self.plan = _hip.Plan(N, prec, max_rows=max_rows, lib=lib, options=options)
        self.bufs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        b = _hip.DeviceBuffer(max(a.nbytes, 16), lib=self.lib)
        self.bufs.append(b)
        b.upload(self.plan, a)
        return b

    def close(self):
        for b in self.bufs:
            b.free()
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run_hop(dev, x, kind, param, sj, hop, output=0, Q=None, alpha=0.0, ld=None, extra_rows=0, fill=None, xhat=None, dt=1.0):
    """cwt_transform_hop of x ((n0,) or (nb, n0)): the whole output matrix ((nb * rows + extra_rows) x ld), prefilled with
    `fill`; xhat: a device buffer that receives the spectra"""
    x = np.atleast_2d(np.asarray(x, dtype=dev.real))
    nb, n0 = x.shape
    nch = -(-n0 // hop)
    ld = nch if ld is None else ld
    dtype = dev.real if output == 1 else dev.cplx
    shape = (nb * len(sj) + extra_rows, ld)
    out = dev.up(np.zeros(shape, dtype=dtype) if fill is None else np.full(shape, fill, dtype=dtype))
    xd = dev.up(x)
    qd = dev.up(np.asarray(Q, dtype=dev.real)) if Q is not None else None
    dev.plan.transform_hop(xd.ptr, nb, n0, n0, kind, param, dt, sj, hop, xhat.ptr if xhat is not None else None, output, out.ptr, ld,
                           qd.ptr if qd is not None else None, alpha)
    return out.download(dev.plan, shape, dtype)


def run_full(dev, x, kind, param, sj, dt=1.0):
    """the existing cwt_transform of one signal: rows x n0"""
    x = np.asarray(x, dtype=dev.real)
    n0 = x.size
    xd, Wd = dev.up(x), dev.up(np.zeros((len(sj), n0), dtype=dev.cplx))
    dev.plan.transform(xd.ptr, n0, kind, param, dt, sj, None, Wd.ptr, n0, n0)
    return Wd.download(dev.plan, (len(sj), n0), dev.cplx)
