"""The caller-side exports of the C ABI (include/cwt_hip.h: the building blocks behind icwt, xwt, wct, Morlet.smooth, the power
reductions, pad=False and the device surrogates), each called directly at strided and ragged shapes on the CPU emulation;
tests/test_exports_gpu.py runs the same case functions on the GPU.

Every case: inputs are nrows x ld matrices with ld > ncols whose padding columns hold NaN (a read of the padding shows in the
result); outputs have ld > ncols and one extra row before and after, all prefilled with a byte pattern that must come back
bit for bit.  The reference is plain NumPy in np.longdouble on the inputs as rounded to the plan's precision -- no call into the
library, no oracle function.  Bounds (eps = machine epsilon of the plan's precision), none of them tuned:
  element-wise exports   4 eps of the reference magnitude of the element (cross terms: of |W1||W2|/s);
  scale reductions       (nrows + 4) eps |coeff| sum_j |w_j g(W_jn)| per column (holds for any summation order);
  time means             (ncols + 4) 2^-53 mean|.| + eps |ref| (fp64 accumulation, one rounding to the plan's type);
  boxcar                 (nwin + 2) eps sum_i |win_i||T|;
  FFT-based exports      the per-row metric conftest.row_errors against TOL of tests/test_gpu_parity.py;
  angle of wct_products  |exp(i got) - exp(i ref)| <= 16 eps (depends on the device library's atan2);
  AR(1) filter           against scipy.signal.lfilter in float64: a term of lag k has gone through k + 1 steps of one multiply and
                         one add in fp64, in the kernel and in lfilter alike: 2 * 2 (k + 1) 2^-53 |g|^k |e[i-k]| summed over k,
                         + the history a segment may forget by design (1e-17, taken as 1e-16 of the largest |g|-filtered |e|)
                         + eps |ref| for the rounding of the output;
  spectrum range         (n + 8) 2^-53 relative (sums of non-negative fp64 terms, any order; the square root halves it);
  histogram, generator   exact."""
import math

import numpy as np
import pytest

from conftest import row_errors
from pycwt_amd import _hip

LD, CLD = np.longdouble, np.clongdouble
TOL = {64: 1e-11, 32: 3e-5}                   # tests/test_gpu_parity.py
EINVAL = -1
GUARD = 0xA5                                  # byte of the prefilled outputs (as a float: a finite, absurd value)
U64 = 2.0 ** -53


def types(precision):
    real, cplx = (np.float64, np.complex128) if precision == 64 else (np.float32, np.complex64)
    return real, cplx, float(np.finfo(real).eps)


def wide(a):
    a = np.asarray(a)
    return a.astype(CLD if np.iscomplexobj(a) else LD)


def crandn(rng, shape, cplx):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cplx)


class Frame:
    """An output matrix on the device: nrows x ld with one guard row before and after, every byte GUARD (`inner`: the first ncols
    columns of the nrows rows hold a matrix, their padding `pad`).  fetch() returns the nrows x ncols block after checking that
    every other byte is what was uploaded."""

    def __init__(self, rig, nrows, ncols, ld, dtype, inner=None, pad=None):
        assert ld > ncols or (ld == ncols and pad is None)       # (ld == ncols: exports whose output has no leading dimension)
        self.rig, self.nrows, self.ncols = rig, nrows, ncols
        self.host = np.empty((nrows + 2, ld), dtype=dtype)
        self.host.view(np.uint8)[...] = GUARD
        if inner is not None:
            self.host[1:-1, :ncols] = inner
            if pad is not None:
                self.host[1:-1, ncols:] = pad
        self.base = rig.dev(self.host)
        self.ptr = self.base + ld * self.host.itemsize

    def fetch(self):
        after = self.rig.download(self.base, self.host.shape, self.host.dtype)
        inner = after[1:-1, :self.ncols].copy()
        after[1:-1, :self.ncols] = self.host[1:-1, :self.ncols]
        assert after.tobytes() == self.host.tobytes(), "bytes outside the nrows x ncols block were written"
        return inner


class Rig:
    """A plan and the device buffers of one case."""

    def __init__(self, lib, nfft, precision, max_rows=8, options=None):
        self.lib = lib
        self.plan = _hip.Plan(nfft, precision, max_rows=max_rows, lib=lib, options=options)
        self.bufs = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        self.plan.close()

    def free(self):
        for b in self.bufs.values():
            b.free()
        self.bufs = {}

    def dev(self, arr):
        arr = np.ascontiguousarray(arr)
        b = _hip.DeviceBuffer(max(arr.nbytes, 8), lib=self.lib)
        b.upload(self.plan, arr)
        self.bufs[b.ptr] = b
        return b.ptr

    def download(self, ptr, shape, dtype):
        return self.bufs[ptr].download(self.plan, shape, dtype)

    def matrix(self, a, ld, pad=np.nan):
        """a (nrows x ncols) as an nrows x ld input matrix on the device, padding columns = pad."""
        a = np.atleast_2d(a)
        assert ld > a.shape[1]
        full = np.full((a.shape[0], ld), pad, dtype=a.dtype)
        full[:, :a.shape[1]] = a
        return self.dev(full)

    def frame(self, nrows, ncols, ld, dtype, inner=None, pad=None):
        return Frame(self, nrows, ncols, ld, dtype, inner, pad)

    def vector(self, n, dtype):
        """An output vector of n elements with guards before and after."""
        return Frame(self, 1, n, n + 1, dtype)


def within(got, ref, bound, what):
    err = np.abs(wide(got) - ref)
    bad = ~(err <= bound)                                     # (a NaN fails)
    assert not bad.any(), (what, float(np.max(np.where(bad, err, 0))), float(np.max(np.where(bad, bound, 0))), int(bad.sum()))


# ---- scale reductions --------------------------------------------------------------------------------------------------------
def _reduce_case(lib, precision):
    """cwt_reduce_scales power 0, 1, 2 and cwt_icwt_reduce: the 8 rows in flight of k_icwt / k_icwt_real and their remainder loop
    (nrows 7 | 8 | 9, 16, 23), the 128-thread blocks and their column tail (ncols 127 | 128 | 129, 300)."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(101)
    coeff = -0.37
    with Rig(lib, 16, precision, max_rows=32) as r:
        for nrows in (1, 7, 8, 9, 16, 23):
            w = rng.standard_normal(nrows)
            if nrows >= 7:
                w[[2, nrows - 1]] = 0.0                           # zeros, at the end of the remainder loop too
                w[3] = -abs(w[3])
            scales = rng.uniform(0.5, 40.0, nrows)
            for ncols in (1, 127, 128, 129, 300):
                W = crandn(rng, (nrows, ncols), cplx)
                P = (rng.standard_normal((nrows, ncols)) ** 2).astype(real)
                ldw, ldp = ncols + 3, ncols + 4                  # (one of them is odd)
                Wd, Pd = r.matrix(W, ldw), r.matrix(P, ldp)
                Wl, Pl = wide(W), wide(P)
                for name, g, wts in (("power0", Wl.real, wide(w)), ("power1", Wl.real ** 2 + Wl.imag ** 2, wide(w)),
                                     ("power2", Pl, wide(w)), ("icwt", Wl.real, 1 / np.sqrt(wide(scales)))):
                    out = r.vector(ncols, real)
                    if name == "icwt":
                        r.plan.icwt_reduce(Wd, ldw, ncols, scales, coeff, out.ptr)
                    elif name == "power2":
                        r.plan.reduce_scales(Pd, ldp, ncols, w, 2, coeff, out.ptr)
                    else:
                        r.plan.reduce_scales(Wd, ldw, ncols, w, int(name[-1]), coeff, out.ptr)
                    terms = wts[:, None] * g
                    within(out.fetch()[0], coeff * terms.sum(axis=0), (nrows + 4) * eps * abs(coeff) * np.abs(terms).sum(axis=0),
                           (name, nrows, ncols))
                r.free()


# ---- time means ----------------------------------------------------------------------------------------------------------------
def _time_mean_case(lib, precision):
    """cwt_time_mean_power / cwt_time_mean_real: the 4 x 256 column unroll (its test n + 3 * 256 < ncols turns at 769 and 1793),
    the tail loop and the LDS tree."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(102)
    with Rig(lib, 16, precision) as r:
        for nrows in (1, 3):
            for ncols in (1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 1100):
                W = crandn(rng, (nrows, ncols), cplx)
                P = (rng.standard_normal((nrows, ncols)) ** 2).astype(real)
                ldw, ldp = ncols + 5, ncols + 2
                Wd, Pd = r.matrix(W, ldw), r.matrix(P, ldp)
                for name, v in (("power", wide(W).real ** 2 + wide(W).imag ** 2), ("real", wide(P))):
                    out = r.vector(nrows, real)
                    if name == "power":
                        r.plan.time_mean_power(Wd, ldw, ncols, nrows, out.ptr)
                    else:
                        r.plan.time_mean_real(Pd, ldp, ncols, nrows, out.ptr)
                    ref = v.mean(axis=1)
                    within(out.fetch()[0], ref, (ncols + 4) * U64 * np.abs(v).mean(axis=1) + eps * np.abs(ref), (name, nrows, ncols))
                r.free()


# ---- element-wise exports ------------------------------------------------------------------------------------------------------
def _abs2_case(lib, precision):
    """cwt_abs2 with ldw != ldp."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(103)
    with Rig(lib, 16, precision) as r:
        for nrows in (1, 5):
            for ncols in (1, 255, 256, 257):
                W = crandn(rng, (nrows, ncols), cplx)
                ldw, ldp = ncols + 3, ncols + 6
                out = r.frame(nrows, ncols, ldp, real)
                r.plan.abs2(r.matrix(W, ldw), ldw, ncols, nrows, out.ptr, ldp)
                ref = wide(W).real ** 2 + wide(W).imag ** 2
                within(out.fetch(), ref, 4 * eps * ref, (nrows, ncols))
                r.free()


def _cross_spectrum_case(lib, precision):
    """cwt_cross_spectrum out of place and with out_dev == W1_dev."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(104)
    nrows = 3
    with Rig(lib, 16, precision) as r:
        for ncols in (1, 255, 257):
            ld = ncols + 2                                           # odd
            W1, W2 = crandn(rng, (nrows, ncols), cplx), crandn(rng, (nrows, ncols), cplx)
            ref = wide(W1) * np.conj(wide(W2))
            bound = 4 * eps * np.abs(wide(W1)) * np.abs(wide(W2))
            W2d = r.matrix(W2, ld)
            out = r.frame(nrows, ncols, ld, cplx)
            r.plan.cross_spectrum(r.matrix(W1, ld), W2d, nrows, ld, ncols, out.ptr)
            within(out.fetch(), ref, bound, ("out of place", ncols))
            io = r.frame(nrows, ncols, ld, cplx, inner=W1, pad=np.nan)
            r.plan.cross_spectrum(io.ptr, W2d, nrows, ld, ncols, io.ptr)
            within(io.fetch(), ref, bound, ("in place", ncols))
            r.free()


def _wct_inputs(rng, nrows, ncols, cplx):
    """Two matrices whose product W1 conj(W2) covers every quadrant and, on planted elements, lies on and just on both sides of the
    negative real axis (the branch cut of the angle)."""
    W1, W2 = crandn(rng, (nrows, ncols), cplx), crandn(rng, (nrows, ncols), cplx)
    tiny = 1e-30 if cplx == np.complex128 else 1e-20
    plant = [(-1.0, 1e-3), (-1.0, -1e-3), (-1.0, tiny), (-1.0, -tiny), (-1.0, 0.0)]       # W2; W1 = 2: W1 conj(W2) = -2 -+ 2i im
    flat1, flat2 = W1.reshape(-1), W2.reshape(-1)
    for i, (re, im) in enumerate(plant[:flat1.size]):
        flat1[-1 - i], flat2[-1 - i] = 2.0, complex(re, im)
    return W1, W2


def _wct_products_case(lib, precision):
    """cwt_wct_products: P = (|W1|^2 + i |W2|^2) / s, C = W1 conj(W2) / s, angle = arg(W1 conj(W2)), one ld for five matrices."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(105)
    nrows = 3
    with Rig(lib, 16, precision) as r:
        for ncols in (1, 255, 257):
            ld = ncols + 2
            W1, W2 = _wct_inputs(rng, nrows, ncols, cplx)
            s = rng.uniform(0.5, 40.0, nrows)
            P, C, A = r.frame(nrows, ncols, ld, cplx), r.frame(nrows, ncols, ld, cplx), r.frame(nrows, ncols, ld, real)
            r.plan.wct_products(r.matrix(W1, ld), r.matrix(W2, ld), s, ld, ncols, P.ptr, C.ptr, A.ptr)
            a, b, sl = wide(W1), wide(W2), wide(s)[:, None]
            p1, p2, c = (a.real ** 2 + a.imag ** 2) / sl, (b.real ** 2 + b.imag ** 2) / sl, a * np.conj(b) / sl
            got = P.fetch()
            within(got.real, p1, 4 * eps * p1, ("P.re", ncols))
            within(got.imag, p2, 4 * eps * p2, ("P.im", ncols))
            within(C.fetch(), c, 4 * eps * np.abs(a) * np.abs(b) / sl, ("C", ncols))
            ang = wide(A.fetch())
            assert np.all(np.abs(ang) <= LD(np.pi) * (1 + eps))
            within(np.exp(1j * ang), np.exp(1j * np.angle(c)), 16 * eps, ("angle", ncols))
            if ncols > 1:
                side = c.imag[np.abs(c.real + 2 / sl.repeat(ncols, 1)) < 1e-2 / sl.repeat(ncols, 1)]
                assert (side > 0).any() and (side < 0).any()          # both sides of the negative real axis were drawn
            r.free()


def _wct_coherence_case(lib, precision):
    """cwt_wct_coherence: |S12|^2 / (S1 S2), S = S1 + i S2."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(106)
    nrows = 3
    with Rig(lib, 16, precision) as r:
        for ncols in (1, 255, 257):
            ld = ncols + 2
            S = (rng.uniform(0.2, 3.0, (nrows, ncols)) + 1j * rng.uniform(0.2, 3.0, (nrows, ncols))).astype(cplx)
            S12 = crandn(rng, (nrows, ncols), cplx)
            out = r.frame(nrows, ncols, ld, real)
            r.plan.wct_coherence(r.matrix(S, ld), r.matrix(S12, ld), nrows, ld, ncols, out.ptr)
            ref = (wide(S12).real ** 2 + wide(S12).imag ** 2) / (wide(S).real * wide(S).imag)
            within(out.fetch(), ref, 4 * eps * ref, ncols)
            r.free()


# ---- boxcar --------------------------------------------------------------------------------------------------------------------
def boxcar_reference(T, win):
    """out[j] = sum_i win[i] T[j + (L - 1) // 2 - i], zero outside: scipy.signal.convolve2d(T, win[:, None], 'same').  Returns
    (sum, sum of the terms' magnitudes)."""
    Tl, wl = wide(T), wide(win)
    nrows, L = Tl.shape[0], wl.size
    out, mag = np.zeros(Tl.shape, CLD), np.zeros(Tl.shape, LD)
    for i in range(L):
        d = (L - 1) // 2 - i                                       # out[j] += win[i] T[j + d]
        lo, hi = max(0, -d), min(nrows, nrows - d)
        if hi > lo:
            out[lo:hi] += wl[i] * Tl[lo + d:hi + d]
            mag[lo:hi] += abs(wl[i]) * np.abs(Tl[lo + d:hi + d])
    return out, mag


def _boxcar_edges_case(lib, precision):
    """cwt_boxcar_scales on both sides of the limit of the LDS ring kernel (nwin 16 | 17 in complex128, 32 | 33 in complex64), of its
    32-row strips (nrows 31 | 32 | 33, 70) and of the matrix (nwin = nrows, nrows + 3), even and odd windows."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(107)
    with Rig(lib, 16, precision, max_rows=80) as r:
        for nrows in (1, 31, 32, 33, 70):
            for ncols in (255, 257):
                ld = ncols + 3
                T = crandn(rng, (nrows, ncols), cplx)
                Td = r.matrix(T, ld)
                for nwin in sorted({1, 2, 3, 15, 16, 17, 31, 32, 33, nrows, nrows + 3}):
                    win = rng.uniform(-1.0, 1.0, nwin)
                    out = r.frame(nrows, ncols, ld, cplx)
                    r.plan.boxcar_scales(Td, nrows, ld, ncols, win, out.ptr)
                    ref, mag = boxcar_reference(T, win)
                    within(out.fetch(), ref, (nwin + 2) * eps * mag, (nrows, ncols, nwin))
                r.free()


# ---- histogram -----------------------------------------------------------------------------------------------------------------
def _histogram_edges_case(lib, precision):
    """cwt_coherence_histogram with ld > the span, an empty row, max_span exactly the longest span, accumulated over two calls.
    The padding and the columns outside [lo, hi) hold countable values (NaNs are skipped: they would hide a read)."""
    real, _, _ = types(precision)
    rng = np.random.default_rng(108)
    rows, ncols, ld = 5, 300, 307
    lo = np.array([0, 17, 150, 299, 4], dtype=np.int64)
    hi = np.array([300, 290, 150, 300, 263], dtype=np.int64)       # the full row (the longest span), interior, empty, 1 column, interior
    with Rig(lib, 16, precision) as r:
        for nbins in (1, 1000, 16384):
            r2 = rng.random((rows, ncols)).astype(real)
            r2[0, ::7] = np.nan
            r2[1, ::5] = 1.0                                       # floor(1.0 * nbins) = nbins: skipped
            r2[3, ::3] = -0.25
            r2d = r.matrix(r2, ld, pad=0.5)
            hist = r.frame(rows, nbins, nbins, np.uint64, inner=0)
            for _ in range(2):
                r.plan.coherence_histogram(r2d, ld, rows, r.dev(lo), r.dev(hi), int((hi - lo).max()), nbins, hist.ptr)
            # (the kernel's own arithmetic: the product in the plan's type, correctly rounded in NumPy as on the device)
            want = np.zeros((rows, nbins), dtype=np.uint64)
            for s in range(rows):
                with np.errstate(invalid="ignore"):
                    v = np.floor(r2[s, lo[s]:hi[s]] * real(nbins))
                want[s] = 2 * np.bincount(v[(v >= 0) & (v < nbins)].astype(int), minlength=nbins)
            np.testing.assert_array_equal(hist.fetch(), want)
            assert want[2].sum() == 0 and want.sum() > 0
            r.free()


# ---- FFT-based exports ---------------------------------------------------------------------------------------------------------
def signed_bins(n):
    k = np.arange(n)
    return np.where(k < (n + 1) // 2, k, k - n)                    # numpy.fft.fftfreq order, even and odd n


def profile(mother, param, f):
    """The real profiles of cwt_filter_rows (include/cwt_hip.h) in longdouble."""
    f = wide(f)
    if mother == _hip.MORLET:
        return np.exp(-(f - LD(param)) ** 2 / 2)
    if mother == _hip.PAUL:
        fp = np.where(f > 0, f, LD(1))
        return np.where(f > 0, fp ** int(param) * np.exp(-fp), LD(0))
    return f ** int(param) * np.exp(-f * f / 2)


def assert_rows(got, ref, precision, what):
    per_row, _ = row_errors(wide(got), ref)
    assert np.all(per_row <= TOL[precision]), (what, float(per_row.max()))


def _fft_rows_case(lib, precision):
    """cwt_fft_rows, real and complex input, in_ld > ncols_in, zero padding from ncols_in to nfft; one single-workgroup length and one
    beyond it (two passes)."""
    real, cplx, _ = types(precision)
    rng = np.random.default_rng(109)
    for nfft in (256, 8192):
        with Rig(lib, nfft, precision) as r:
            for nrows in (1, 3):
                for ncols_in in (1, nfft - 3, nfft):
                    in_ld = ncols_in + 5
                    for is_cplx in (False, True):
                        x = crandn(rng, (nrows, ncols_in), cplx) if is_cplx else rng.standard_normal((nrows, ncols_in)).astype(real)
                        out = r.frame(nrows, nfft, nfft, cplx)
                        r.plan.fft_rows(r.matrix(x, in_ld), is_cplx, nrows, in_ld, ncols_in, out.ptr)
                        assert_rows(out.fetch(), np.fft.fft(wide(x), n=nfft, axis=1), precision, (nfft, nrows, ncols_in, is_cplx))
                        r.free()


def _filter_rows_case(lib, precision):
    """cwt_filter_rows: one shared spectrum (spec_ld = 0) against per-row spectra (spec_ld = nfft), ncols < nfft, ldw > ncols, complex
    amplitudes, the three profiles."""
    real, cplx, _ = types(precision)
    rng = np.random.default_rng(110)
    nrows = 3
    for nfft in (256, 8192):
        ncols = nfft - 5
        ldw = ncols + 3
        sk = signed_bins(nfft)
        sk[nfft // 2] = -(nfft // 2)                               # (the header's order: k - nfft for k >= nfft / 2)
        with Rig(lib, nfft, precision) as r:
            spec = crandn(rng, (nrows, nfft), cplx)
            specd = r.dev(spec)
            for mother, param, peak in ((_hip.MORLET, 6.0, 6.0), (_hip.PAUL, 4, 4.0), (_hip.DOG, 2, math.sqrt(2.0))):
                a = peak / (nfft * np.array([1 / 8, 1 / 23, 1 / 3.3]))           # filter peaks at bins nfft / 8, / 23, / 3.3
                amp = np.array([0.7 - 1.1j, -0.2 + 0.9j, 1.3 + 0.4j])
                for spec_ld in (0, nfft):
                    out = r.frame(nrows, ncols, ldw, cplx)
                    r.plan.filter_rows(specd, spec_ld, mother, param, a, amp, out.ptr, ldw, ncols)
                    src = wide(spec) if spec_ld else np.repeat(wide(spec[:1]), nrows, axis=0)
                    F = wide(amp)[:, None] * profile(mother, param, wide(a)[:, None] * wide(sk)[None, :])
                    assert_rows(out.fetch(), np.fft.ifft(src * F, axis=1)[:, :ncols], precision, (nfft, mother, spec_ld))


def _table_case(lib, precision):
    """cwt_transform_rows_table: a filter bank of the caller's with signed-bin supports -- across bin 0, one bin, touching -nfft / 2,
    everything; the table holds NaN outside a row's support (those bins count as exactly zero)."""
    real, cplx, _ = types(precision)
    rng = np.random.default_rng(111)
    nfft, ncols = 256, 200
    ldw = ncols + 3
    k_lo = np.array([-20, 5, -128, -128, 3, -7], dtype=np.int32)
    nband = np.array([41, 1, 10, 256, 50, 1], dtype=np.int32)
    rows = k_lo.size
    sk = signed_bins(nfft)
    sk[nfft // 2] = -(nfft // 2)
    with Rig(lib, nfft, precision) as r:
        xhat = crandn(rng, nfft, cplx)
        bank = crandn(rng, (rows, nfft), cplx)
        live = (sk[None, :] >= k_lo[:, None]) & (sk[None, :] < (k_lo + nband)[:, None])
        table = np.where(live, bank, np.nan + 1j * np.nan).astype(cplx)
        out = r.frame(rows, ncols, ldw, cplx)
        r.plan.transform_rows_table(r.dev(xhat), r.dev(table), k_lo, nband, out.ptr, ldw, ncols)
        F = np.where(live, wide(bank), CLD(0))
        assert_rows(out.fetch(), np.fft.ifft(wide(xhat)[None, :] * F, axis=1)[:, :ncols], precision, "table")


def mother_psi_ft_bar(mother, param, f):
    """conj(psi_ft(f)) of pycwt's Morlet / Paul / DOG (Torrence & Compo 1998, table 1) in longdouble."""
    m = int(param)
    if mother == _hip.MORLET:
        return LD(np.pi) ** LD(-0.25) * profile(mother, param, f)
    if mother == _hip.PAUL:
        return LD(2) ** m / np.sqrt(LD(m * math.factorial(2 * m - 1))) * profile(mother, param, f)
    return np.conj(-(CLD(1j) ** m)) / np.sqrt(LD(math.gamma(m + 0.5))) * profile(mother, param, f)


def _bluestein_case(lib, precision):
    """cwt_forward_fft_n + cwt_transform_rows_n: transform lengths that are no power of two (odd, even, prime, and 128), ldw > n0, more
    rows than the plan's max_rows (the slab loop runs three times)."""
    real, cplx, _ = types(precision)
    rng = np.random.default_rng(112)
    dt, nrows = 0.25, 5
    for n0 in (3, 128, 331, 504):
        nfft = 1 << int(2 * n0 - 2).bit_length()                   # smallest power of two >= 2 n0 - 1
        assert nfft >= 2 * n0 - 1 > nfft // 2
        ldw = n0 + 3
        x = rng.standard_normal(n0).astype(real)
        n = np.arange(n0)
        dft = np.exp(-2j * LD(np.pi) * wide((n[:, None] * n[None, :]) % n0) / n0)
        xhat = dft @ wide(x)
        w = 2 * LD(np.pi) * wide(signed_bins(n0)) / (n0 * LD(dt))
        scales = dt * np.array([0.4, 0.7, 1.1, 1.6, 2.2])       # (every profile is alive on the three bins of n0 = 3 too)
        with Rig(lib, nfft, precision, max_rows=2) as r:
            xh = r.vector(n0, cplx)
            r.plan.forward_fft_n(r.dev(x), n0, xh.ptr)
            assert_rows(xh.fetch(), xhat[None, :], precision, ("forward", n0))
            for mother, param in ((_hip.MORLET, 6.0), (_hip.PAUL, 4), (_hip.DOG, 1)):
                out = r.frame(nrows, n0, ldw, cplx)
                r.plan.transform_rows_n(xh.ptr, n0, mother, param, dt, scales, out.ptr, ldw)
                sl = wide(scales)[:, None]
                F = np.sqrt(sl * w[1] * n0) * mother_psi_ft_bar(mother, param, sl * w[None, :])
                ref = (np.conj(dft) @ (xhat[None, :] * F).T).T / n0
                assert_rows(out.fetch(), ref, precision, (n0, mother))


# ---- surrogates and the spectrum range -------------------------------------------------------------------------------------------
AR1_ROWS = [(0.0, 0, 1), (0.5, 0, 63), (0.5, 1000, 65), (0.99, 10, 5000), (-0.999, 0, 20000), (0.9999, 3, 300)]


def _ar1_case(lib, precision):
    """cwt_ar1_filter for (g, tau, n) that put the host's choice of segment and warm-up on its edges, against scipy.signal.lfilter in
    float64 on the rounded input (bound: module docstring).  What no bound can see: a warm-up one sample shorter -- the sample it
    drops weighs g^warm <= 1e-17 by construction, and where the warm-up is clipped at e[0] nothing is dropped."""
    from scipy.signal import lfilter
    real, _, eps = types(precision)
    rng = np.random.default_rng(113)
    with Rig(lib, 16, precision) as r:
        for g, tau, n in AR1_ROWS:
            e = rng.standard_normal(tau + n).astype(real)
            out = r.vector(n, real)
            r.plan.ar1_filter(r.matrix(e[None, :], tau + n + 1), tau, n, g, out.ptr)
            e64 = e.astype(np.float64)
            ref = lfilter([1, 0], [1, -g], e64)[tau:]
            S = lfilter([1], [1, -abs(g)], np.abs(e64))            # sum_k |g|^k |e[i-k]|
            B = lfilter([1], [1, -abs(g)], S)                      # sum_k (k + 1) |g|^k |e[i-k]|
            bound = 4 * U64 * B[tau:] + 1e-16 * S.max() + eps * np.abs(ref)
            within(out.fetch()[0], wide(ref), bound, (g, tau, n))
            r.free()


def _random_normal_case(lib, precision):
    """cwt_random_normal at odd and even n: nothing past n is written, and the first n values are the prefix of a longer draw with the
    same seed and offset, bit for bit."""
    real, _, _ = types(precision)
    seed, offset = 0x1234567890ABCDEF, (1 << 40) + 3
    with Rig(lib, 16, precision) as r:
        long_draw = r.vector(1024, real)
        r.plan.random_normal(seed, offset, 1024, 1.5, long_draw.ptr)
        ref = long_draw.fetch()[0]
        assert np.isfinite(ref).all() and 0.5 < ref.std() / 1.5 < 1.5
        for n in (1, 2, 255, 513):
            out = r.vector(n, real)
            r.plan.random_normal(seed, offset, n, 1.5, out.ptr)
            assert out.fetch()[0].tobytes() == ref[:n].tobytes(), n


def spectrum_range_reference(x):
    """max|x|, rms|x| and the rms of the quietest run of three neighbouring non-empty quarter-octave windows of the positive half
    (include/cwt_hip.h: cwt_spectrum_range), in longdouble."""
    n = x.size
    p = wide(x).real ** 2 + wide(x).imag ** 2
    windows, w = [], 0
    while True:
        b, q = w >> 2, w & 3
        lo = ((1 << b) * (4 + q) + 3) >> 2
        if lo >= n // 2:
            break
        hi = min(((1 << ((w + 1) >> 2)) * (4 + ((w + 1) & 3)) + 3) >> 2, n // 2)
        if hi > lo:
            windows.append((p[lo:hi].sum(), hi - lo))
        w += 1
    floors = []
    for i in range(len(windows)):
        near = windows[max(i - 1, 0):i + 2]
        floors.append(np.sqrt(sum(e for e, _ in near) / sum(c for _, c in near)))
    rms = np.sqrt(p.sum() / n)
    return np.sqrt(p.max()), rms, (min(floors) if floors else rms)


def _spectrum_range_case(lib, precision):
    real, cplx, _ = types(precision)
    rng = np.random.default_rng(114)
    with Rig(lib, 16, precision) as r:
        for n in (2, 8, 5000):
            x = crandn(rng, n, cplx) * np.linspace(1.0, 30.0, n).astype(real)
            got = r.plan.spectrum_range(r.matrix(x[None, :], n + 1), n)
            for name, g, want in zip(("max", "rms", "floor"), got, spectrum_range_reference(x)):
                assert abs(LD(g) - want) <= (n + 8) * U64 * want, (n, name, g, float(want))
            r.free()


# ---- rows beyond the grid limit ------------------------------------------------------------------------------------------------
def _row_limit_case(lib, precision):
    """gridDim.y is limited to 65535.  cwt_wct_products, cwt_wct_coherence, cwt_boxcar_scales and cwt_coherence_histogram take any
    nrows (include/cwt_hip.h): 65539 rows go out in slabs, and the boxcar's taps reach across the slabs' edges.  The emulation accepts
    any grid, so it checks the slabs' offsets; the limit itself is checked where this runs on the GPU."""
    real, cplx, eps = types(precision)
    rng = np.random.default_rng(115)
    nrows, ncols, ld = 65539, 5, 6
    with Rig(lib, 2, precision, max_rows=nrows) as r:
        W1, W2 = _wct_inputs(rng, nrows, ncols, cplx)
        s = rng.uniform(0.5, 40.0, nrows)
        W1d, W2d = r.matrix(W1, ld), r.matrix(W2, ld)
        P, C, A = r.frame(nrows, ncols, ld, cplx), r.frame(nrows, ncols, ld, cplx), r.frame(nrows, ncols, ld, real)
        r.plan.wct_products(W1d, W2d, s, ld, ncols, P.ptr, C.ptr, A.ptr)
        a, b, sl = wide(W1), wide(W2), wide(s)[:, None]
        p1, p2, c = (a.real ** 2 + a.imag ** 2) / sl, (b.real ** 2 + b.imag ** 2) / sl, a * np.conj(b) / sl
        got = P.fetch()
        within(got.real, p1, 4 * eps * p1, "P.re")
        within(got.imag, p2, 4 * eps * p2, "P.im")
        within(C.fetch(), c, 4 * eps * np.abs(a) * np.abs(b) / sl, "C")
        within(np.exp(1j * wide(A.fetch())), np.exp(1j * np.angle(c)), 16 * eps, "angle")
        r.free()

        S = (rng.uniform(0.2, 3.0, (nrows, ncols)) + 1j * rng.uniform(0.2, 3.0, (nrows, ncols))).astype(cplx)
        out = r.frame(nrows, ncols, ld, real)
        r.plan.wct_coherence(r.matrix(S, ld), r.matrix(W1, ld), nrows, ld, ncols, out.ptr)
        ref = (a.real ** 2 + a.imag ** 2) / (wide(S).real * wide(S).imag)
        within(out.fetch(), ref, 4 * eps * ref, "coherence")
        r.free()

        for nwin in (33,):                                         # the plain kernel in both precisions
            win = rng.uniform(-1.0, 1.0, nwin)
            out = r.frame(nrows, ncols, ld, cplx)
            r.plan.boxcar_scales(r.matrix(W2, ld), nrows, ld, ncols, win, out.ptr)
            ref, mag = boxcar_reference(W2, win)
            within(out.fetch(), ref, (nwin + 2) * eps * mag, ("boxcar", nwin))
            r.free()

        nbins = 8
        r2 = rng.random((nrows, ncols)).astype(real)
        lo = rng.integers(0, 3, nrows).astype(np.int64)
        hi = (lo + rng.integers(0, 4, nrows)).astype(np.int64)     # spans of 0 ... 3 columns inside the 5
        hi[7] = lo[7] + 3
        hist = r.dev(np.zeros((nrows, nbins), dtype=np.uint64))
        r.plan.coherence_histogram(r.matrix(r2, ld, pad=0.5), ld, nrows, r.dev(lo), r.dev(hi), 3, nbins, hist)
        col = np.arange(ncols)[None, :]
        v = np.floor(r2 * real(nbins)).astype(int)
        inside = (col >= lo[:, None]) & (col < hi[:, None]) & (v >= 0) & (v < nbins)
        want = np.zeros((nrows, nbins), dtype=np.uint64)
        np.add.at(want, (np.nonzero(inside)[0], v[inside]), 1)
        np.testing.assert_array_equal(r.download(hist, (nrows, nbins), np.uint64), want)


CASES = {"reduce_scales_and_icwt": _reduce_case, "time_means": _time_mean_case, "abs2": _abs2_case,
         "cross_spectrum": _cross_spectrum_case, "wct_products": _wct_products_case, "wct_coherence": _wct_coherence_case,
         "boxcar_scales": _boxcar_edges_case, "coherence_histogram": _histogram_edges_case, "fft_rows": _fft_rows_case,
         "filter_rows": _filter_rows_case, "transform_rows_table": _table_case, "bluestein": _bluestein_case,
         "ar1_filter": _ar1_case, "random_normal": _random_normal_case, "spectrum_range": _spectrum_range_case,
         "row_limit": _row_limit_case}


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("export", list(CASES))
def test_export_at_its_edges(emu_library, export, precision):
    CASES[export](emu_library, precision)


# ---- rejections ----------------------------------------------------------------------------------------------------------------
def rejections(plan):
    """(label, call) pairs that must fail with CWT_EINVAL before anything is launched: the addresses are never dereferenced."""
    A, B, C3, D, E = (1 << 20) + 64, (2 << 20) + 64, (3 << 20) + 64, (4 << 20) + 64, (5 << 20) + 64
    one, none = np.ones(2), np.ones(0)
    k2, k0 = np.zeros(2, np.int32), np.zeros(0, np.int32)
    p = plan
    out = []
    for what, ld, ncols in (("ld < ncols", 7, 8), ("ncols < 1", 8, 0)):
        out += [
            ("reduce_scales " + what, lambda ld=ld, ncols=ncols: p.reduce_scales(A, ld, ncols, one, 0, 1.0, B)),
            ("reduce_scales power 2 " + what, lambda ld=ld, ncols=ncols: p.reduce_scales(A, ld, ncols, one, 2, 1.0, B)),
            ("icwt_reduce " + what, lambda ld=ld, ncols=ncols: p.icwt_reduce(A, ld, ncols, one, 1.0, B)),
            ("time_mean_power " + what, lambda ld=ld, ncols=ncols: p.time_mean_power(A, ld, ncols, 2, B)),
            ("time_mean_real " + what, lambda ld=ld, ncols=ncols: p.time_mean_real(A, ld, ncols, 2, B)),
            ("abs2 ldw " + what, lambda ld=ld, ncols=ncols: p.abs2(A, ld, ncols, 2, B, 8)),
            ("abs2 ldp " + what, lambda ld=ld, ncols=ncols: p.abs2(A, 8, ncols, 2, B, ld)),
            ("cross_spectrum " + what, lambda ld=ld, ncols=ncols: p.cross_spectrum(A, B, 2, ld, ncols, C3)),
            ("wct_products " + what, lambda ld=ld, ncols=ncols: p.wct_products(A, B, one, ld, ncols, C3, D, E)),
            ("wct_coherence " + what, lambda ld=ld, ncols=ncols: p.wct_coherence(A, B, 2, ld, ncols, C3)),
            ("boxcar_scales " + what, lambda ld=ld, ncols=ncols: p.boxcar_scales(A, 2, ld, ncols, one, B)),
            ("fft_rows " + what, lambda ld=ld, ncols=ncols: p.fft_rows(A, False, 2, ld, ncols, B)),
            ("filter_rows " + what, lambda ld=ld, ncols=ncols: p.filter_rows(A, 0, _hip.DOG, 0.0, one, 1.0, B, ld, ncols)),
            ("transform_rows_table " + what, lambda ld=ld, ncols=ncols: p.transform_rows_table(A, B, k2, k2 + 1, C3, ld, ncols)),
            ("transform_rows_n " + what, lambda ld=ld, ncols=ncols: p.transform_rows_n(A, ncols, _hip.MORLET, 6.0, 1.0, one, B, ld)),
        ]
    out += [
        ("reduce_scales nrows < 1", lambda: p.reduce_scales(A, 8, 8, none, 0, 1.0, B)),
        ("icwt_reduce nrows < 1", lambda: p.icwt_reduce(A, 8, 8, none, 1.0, B)),
        ("time_mean_power nrows < 1", lambda: p.time_mean_power(A, 8, 8, 0, B)),
        ("time_mean_real nrows < 1", lambda: p.time_mean_real(A, 8, 8, 0, B)),
        ("abs2 nrows < 1", lambda: p.abs2(A, 8, 8, 0, B, 8)),
        ("cross_spectrum nrows < 1", lambda: p.cross_spectrum(A, B, 0, 8, 8, C3)),
        ("wct_products nrows < 1", lambda: p.wct_products(A, B, none, 8, 8, C3, D, E)),
        ("wct_coherence nrows < 1", lambda: p.wct_coherence(A, B, 0, 8, 8, C3)),
        ("boxcar_scales nrows < 1", lambda: p.boxcar_scales(A, 0, 8, 8, one, B)),
        ("boxcar_scales in place", lambda: p.boxcar_scales(A, 2, 8, 8, one, A)),
        ("coherence_histogram nrows < 1", lambda: p.coherence_histogram(A, 8, 0, B, C3, 8, 10, D)),
        ("coherence_histogram ld < 1", lambda: p.coherence_histogram(A, 0, 2, B, C3, 8, 10, D)),
        ("coherence_histogram nbins < 1", lambda: p.coherence_histogram(A, 8, 2, B, C3, 8, 0, D)),
        ("fft_rows nrows < 1", lambda: p.fft_rows(A, False, 0, 8, 8, B)),
        ("fft_rows ncols_in > nfft", lambda: p.fft_rows(A, False, 2, 40, 33, B)),
        ("filter_rows nrows < 1", lambda: p.filter_rows(A, 0, _hip.DOG, 0.0, none, 1.0, B, 8, 8)),
        ("filter_rows 0 < spec_ld < nfft", lambda: p.filter_rows(A, 8, _hip.DOG, 0.0, one, 1.0, B, 8, 8)),
        ("transform_rows_table nrows < 1", lambda: p.transform_rows_table(A, B, k0, k0, C3, 8, 8)),
        ("forward_fft_n n0 < 1", lambda: p.forward_fft_n(A, 0, B)),
        ("forward_fft_n nfft < 2 n0 - 1", lambda: p.forward_fft_n(A, 17, B)),
        ("transform_rows_n nrows < 1", lambda: p.transform_rows_n(A, 8, _hip.MORLET, 6.0, 1.0, none, B, 8)),
        ("ar1_filter n < 1", lambda: p.ar1_filter(A, 0, 0, 0.5, B)),
        ("ar1_filter in place", lambda: p.ar1_filter(A, 0, 8, 0.5, A)),
        ("random_normal n < 1", lambda: p.random_normal(1, 0, 0, 1.0, A)),
        ("spectrum_range n < 1", lambda: p.spectrum_range(A, 0)),
    ]
    return out


def _rejection_case(lib, precision):
    plan = _hip.Plan(32, precision, max_rows=4, lib=lib)
    try:
        for label, call in rejections(plan):
            with pytest.raises(_hip.HipError) as e:
                call()
            assert e.value.code == EINVAL, (label, e.value.code)
    finally:
        plan.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_bad_shapes_are_refused_before_any_launch(emu_library, precision):
    _rejection_case(emu_library, precision)
