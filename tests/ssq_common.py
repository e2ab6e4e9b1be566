"""Shared by tests/test_ssq_emulated.py, tests/test_ssq_gpu.py and tests/test_ssq_schedules_emulated.py: the definition of the
synchrosqueezed transform (include/cwt_hip.h, cwt_ssq_reassign) restated in NumPy, and the cases run against it.

The reference (pycwt) has no synchrosqueezing, so the yardstick is the definition itself:
  decisions   a2, q in the plan's real type T with every operation rounded once (NumPy's float32 / float64 arithmetic is exactly
              that), pos and k in double, kept iff a2 > gamma^2, q finite and > 0, 0 <= k < nf;
  sums        T[k, n] = sum over the kept entries of the cell of w_j W[j, n], in long double from the unrounded weights.
BOUND per cell with m entries: |T - ref| <= (m + 3) eps_T sum |w_j W[j, n]| -- m - 1 additions, one product and the weight's
rounding to T, each half an eps_T of the running magnitude per real component, sqrt(2) for the modulus: (m + 1) / sqrt(2) eps_T at
first order, below (m + 3) eps_T.  A cell without entries is exactly 0.  The oracle (oracle/cwt_oracle.py) serves for W and dW.
"""
import ctypes as C

import numpy as np

from oracle import cwt_oracle as orc
from pycwt_amd import _hip

L = np.longdouble
EINVAL = -1
SENTINEL = -7 - 7j
MOTHERS = {"morlet": (orc.MORLET, 6.0), "paul": (orc.PAUL, 4.0)}
PRECS = (64, 32)


def types(prec):
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    return real, cplx, float(np.finfo(real).eps)


def launch_log(lib):
    """the kernels the emulated library has launched since hipemu_clear_launched()"""
    dll = lib.dll
    dll.hipemu_launched.restype = C.c_size_t
    dll.hipemu_launched.argtypes = [C.c_char_p, C.c_size_t]
    need = dll.hipemu_launched(None, 0)
    buf = C.create_string_buffer(need)
    dll.hipemu_launched(buf, need)
    return set(buf.value.decode().split("\n")) - {""}


class Dev:
    """a plan and the device buffers of a case, freed together"""
    def __init__(self, lib, nfft, prec, max_rows, options=None):
        self.lib, self.prec = lib, prec
        self.real, self.cplx, self.eps = types(prec)
        self.plan = _hip.Plan(nfft, prec, max_rows=max_rows, lib=lib, options=options or {})
        self.bufs = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        b = _hip.DeviceBuffer(max(a.nbytes, 16), lib=self.lib)
        self.bufs.append(b)
        b.upload(self.plan, a)
        return b

    def release(self):
        """the buffers of a case; the plan stays"""
        for b in self.bufs:
            b.free()
        self.bufs = []

    def close(self):
        self.release()
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the definition --------------------------------------------------------------------------------------------------------------
def decisions(W, dW, gamma, f_lo, dv, nf):
    """(kept, k, pos, a2) of every entry; W, dW complex arrays of the plan's precision"""
    re, im, dre, dim = W.real, W.imag, dW.real, dW.imag
    with np.errstate(all="ignore"):
        a2 = re * re + im * im
        q = (dim * re - dre * im) / a2
        pos = np.log2(q.astype(np.float64) / (2 * np.pi * f_lo)) / dv
        kf = np.floor(pos + 0.5)
        kept = (a2.astype(np.float64) > gamma * gamma) & np.isfinite(q) & (q > 0) & (kf >= 0) & (kf < nf)
    return kept, np.where(kept, kf, -1).astype(np.int64), pos, a2


class Reference:
    """the sums of the definition in long double: re, im (nf x ncols), mag = sum |w_j W|, m = entries per cell"""
    def __init__(self, W, dW, w, gamma, f_lo, dv, nf):
        self.kept, self.k, self.pos, self.a2 = decisions(W, dW, gamma, f_lo, dv, nf)
        rows, ncols = W.shape
        self.gamma, self.nf = gamma, nf
        self.re, self.im, self.mag = (np.zeros((nf, ncols), dtype=L) for _ in range(3))
        self.m = np.zeros((nf, ncols), dtype=np.int64)
        cols = np.arange(ncols)
        for j in range(rows):                              # (a column holds a row once: plain fancy-index updates are safe)
            c, kk, wj = cols[self.kept[j]], self.k[j, self.kept[j]], L(w[j])
            vr, vi = W.real[j, c].astype(L), W.imag[j, c].astype(L)
            self.re[kk, c] += wj * vr
            self.im[kk, c] += wj * vi
            self.mag[kk, c] += abs(wj) * np.hypot(vr, vi)
            self.m[kk, c] += 1

    def bound(self, eps, extra_mag=0, extra_m=0):
        return (self.m + extra_m + 3) * L(eps) * (self.mag + extra_mag)

    def doubtful_cells(self, edge=1e-6, rel_gamma=1e-6):
        """cells that an entry within `edge` bins of a bin edge, or within `rel_gamma` relative of gamma, could reach or leave"""
        nf, ncols = self.m.shape
        bad = np.zeros((nf, ncols), dtype=bool)
        with np.errstate(all="ignore"):
            amp = np.sqrt(self.a2.astype(np.float64))
            near_gamma = np.abs(amp - self.gamma) <= rel_gamma * self.gamma if self.gamma > 0 else np.zeros(amp.shape, dtype=bool)
            frac = self.pos + 0.5 - np.floor(self.pos + 0.5)
            near_edge = np.isfinite(self.pos) & ((frac < edge) | (frac > 1 - edge))
            lo, hi = np.floor(self.pos + 0.5 - edge), np.floor(self.pos + 0.5 + edge)
        for j, n in zip(*np.nonzero(near_gamma | near_edge)):
            for kk in {lo[j, n], hi[j, n]}:
                if np.isfinite(kk) and 0 <= kk < nf:
                    bad[int(kk), n] = True
        return bad

    def column_sums(self):
        return self.re.sum(axis=0), self.im.sum(axis=0), self.mag.sum(axis=0), self.m.sum(axis=0)


def assert_cells(T, ref, eps, where=None, extra_mag=0, extra_m=0, base=None):
    """every cell (of `where`) within the bound; base: what T held before an accumulating call"""
    want_re, want_im = (ref.re, ref.im) if base is None else (ref.re + base.real.astype(L), ref.im + base.imag.astype(L))
    err = np.hypot(T.real.astype(L) - want_re, T.imag.astype(L) - want_im)
    bad = err > ref.bound(eps, extra_mag, extra_m)
    if where is not None:
        bad &= where
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), float(err[bad].max()))


def assert_column_sums(T, ref, eps):
    """sum_k T[k, n] = sum over the kept entries of the column, within the bound of the column's entries: T's cells carry (m_k + 3)
    eps of their own magnitudes, the sum over the nf cells adds nf - 1 additions of numbers bounded by the column's magnitude --
    done here in long double, so only the cells' own bounds count"""
    re, im, mag, m = ref.column_sums()
    err = np.hypot(T.real.astype(L).sum(axis=0) - re, T.imag.astype(L).sum(axis=0) - im)
    bound = ref.bound(eps).sum(axis=0)
    assert (err <= bound).all(), (int((err > bound).sum()), float((err / np.where(bound > 0, bound, 1)).max()))


# ---- cwt_ssq_reassign on synthetic matrices ---------------------------------------------------------------------------------------
ROWS, NCOLS, NFS = (1, 8, 13, 64), (1, 127, 129, 1000), (1, 5, 40)
GAMMA, F_LO, DV = 0.5, 0.01, 1.0 / 12
KINDS = {3: "negative", 7: "zero", 11: "nan_w", 13: "nan_dw", 17: "small", 19: "below", 21: "above"}


def synthetic(seed, rows, ncols, nf, prec):
    """W, dW = (a + 2 pi i f) W with |a| <= 2 pi f, f = f_lo 2^((bin + jitter) dv), |jitter| <= 0.25: every kept entry sits >= 0.25
    bin from an edge.  Along j the target bins of a column come in runs of 1, 2 and 9 equal bins (a run of 9 crosses the kernel's 8
    rows in flight), bins revisited.  Planted by position (flat index mod 23): q < 0, W = 0, NaN in W, NaN in dW, |W| = gamma / 2
    with |W| = 2 gamma in the row below, target bins -1 and nf."""
    real, cplx, eps = types(prec)
    rng = np.random.default_rng(seed)
    run_of = []
    while len(run_of) < rows:
        run_of += [len(set(run_of))] * int(rng.choice([1, 2, 9]))
    run_of = np.array(run_of[:rows])
    tk = rng.integers(0, nf, size=(run_of.max() + 1, ncols))[run_of]            # (rows, ncols): equal along a run
    kind = (np.arange(rows)[:, None] * ncols + np.arange(ncols)[None, :]) % 23
    tk = np.where(kind == 19, -1, np.where(kind == 21, nf, tk))
    f = F_LO * 2.0 ** ((tk + rng.uniform(-0.25, 0.25, size=tk.shape)) * DV)
    f = np.where(kind == 3, -f, f)
    amp = GAMMA * rng.uniform(2.0, 10.0, size=tk.shape)
    amp[kind == 17] = GAMMA / 2
    below = np.zeros_like(kind, dtype=bool)
    below[1:] = kind[:-1] == 17
    amp[below & (kind != 17)] = 2 * GAMMA
    amp[kind == 7] = 0.0
    W = (amp * np.exp(2j * np.pi * rng.random(tk.shape))).astype(cplx)
    a = rng.uniform(-1, 1, size=tk.shape) * 2 * np.pi * np.abs(f)
    dW = ((a + 2j * np.pi * f) * W.astype(np.complex128)).astype(cplx)
    W[kind == 11] = complex(np.nan, 1.0)
    dW[kind == 13] = complex(1.0, np.nan)
    w = rng.uniform(0.2, 2.0, size=rows)
    ref = Reference(W, dW, w, GAMMA, F_LO, DV, nf)
    frac = ref.pos[ref.kept] + 0.5 - np.floor(ref.pos[ref.kept] + 0.5)
    assert ((frac > 0.2) & (frac < 0.8)).all()                                  # the construction, not the code under test
    ok = ~np.isin(kind, list(KINDS)) | (below & (kind == 17))
    assert np.array_equal(ref.kept | ~ok, np.ones_like(ok)) and not ref.kept[np.isin(kind, list(KINDS)) & ~below].any()
    return W, dW, w, ref


def padded(A, pad, fill):
    out = np.full((A.shape[0], A.shape[1] + pad), fill, dtype=A.dtype)
    out[:, :A.shape[1]] = A
    return out


def run_reassign(dev, W, dW, w, nf, gamma=GAMMA, f_lo=F_LO, dv=DV, pad=3, chunks=None, T0=None):
    """cwt_ssq_reassign over the rows in chunks of `chunks` rows (None: one call), ld = ldt = ncols + pad, the padding of W and dW
    NaN; T starts as T0 (then every call accumulates) or as the sentinel (the first call zero-fills).  Returns T with its padding."""
    rows, ncols = W.shape
    ld = ncols + pad
    nan = complex(np.nan, np.nan)
    Wd, dWd = dev.up(padded(W, pad, nan)), dev.up(padded(dW, pad, nan))
    start = np.full((nf, ld), SENTINEL, dtype=dev.cplx)
    if T0 is not None:
        start[:, :ncols] = T0
    Td = dev.up(start)
    cs = np.dtype(dev.cplx).itemsize
    step = chunks or rows
    for a in range(0, rows, step):
        b = min(rows, a + step)
        dev.plan.ssq_reassign(Wd.ptr + a * ld * cs, dWd.ptr + a * ld * cs, ld, ncols, w[a:b], gamma, f_lo, dv, nf, Td.ptr, ld,
                              accumulate=T0 is not None or a > 0)
    T = Td.download(dev.plan, (nf, ld), dev.cplx)
    assert np.array_equal(Wd.download(dev.plan, (rows, ld), dev.cplx), padded(W, pad, nan), equal_nan=True)      # inputs are inputs
    dev.release()
    return T


def check_synthetic(dev, rows, ncols, nf):
    W, dW, w, ref = synthetic(1000 * rows + 10 * nf + ncols, rows, ncols, nf, dev.prec)
    T = run_reassign(dev, W, dW, w, nf)
    assert np.all(T[:, ncols:] == SENTINEL)
    assert_cells(T[:, :ncols], ref, dev.eps)
    assert np.all(T[:, :ncols][ref.m == 0] == 0)
    return T


def check_chunks_and_accumulate(dev, rows=13, ncols=129, nf=5):
    W, dW, w, ref = synthetic(77, rows, ncols, nf, dev.prec)
    whole = run_reassign(dev, W, dW, w, nf)
    for chunks in (1, 5):
        assert np.array_equal(run_reassign(dev, W, dW, w, nf, chunks=chunks).view(dev.real), whole.view(dev.real)), chunks
    rng = np.random.default_rng(5)
    T0 = (rng.standard_normal((nf, ncols)) + 1j * rng.standard_normal((nf, ncols))).astype(dev.cplx)
    T = run_reassign(dev, W, dW, w, nf, T0=T0)
    assert np.all(T[:, ncols:] == SENTINEL)
    assert_cells(T[:, :ncols], ref, dev.eps, extra_mag=np.abs(T0).astype(L), extra_m=1, base=T0)      # T0: one more entry of the cell
    assert np.array_equal(T[:, :ncols][ref.m == 0], T0[ref.m == 0])


def refusals(dev, rows=8, ncols=127, nf=5):
    """(label, return code, T after the call) of every argument set cwt_ssq_reassign and cwt_spectrum_derivative refuse"""
    W, dW, w, _ = synthetic(3, rows, ncols, nf, dev.prec)
    ld = ncols + 3
    cs = np.dtype(dev.cplx).itemsize
    Wd, dWd = dev.up(padded(W, 3, 0)), dev.up(padded(dW, 3, 0))
    start = np.full((max(nf, rows), ld), SENTINEL, dtype=dev.cplx)
    Td = dev.up(start)
    lib, h, P = dev.lib, dev.plan.h, C.c_void_p
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(W=Wd.ptr, dW=dWd.ptr, ld=ld, ncols=ncols, nrows=rows, w=wp, gamma=GAMMA, f_lo=F_LO, dv=DV, nf=nf, T=Td.ptr, ldt=ld)
    bad = {"W NULL": dict(W=None), "dW NULL": dict(dW=None), "T NULL": dict(T=None), "weights NULL": dict(w=None),
           "nrows 0": dict(nrows=0), "nrows > max_rows": dict(nrows=dev.plan.max_rows + 1), "ncols 0": dict(ncols=0),
           "ld < ncols": dict(ld=ncols - 1), "ldt < ncols": dict(ldt=ncols - 1), "nf 0": dict(nf=0),
           "gamma nan": dict(gamma=np.nan), "gamma inf": dict(gamma=np.inf), "gamma < 0": dict(gamma=-1.0),
           "f_lo 0": dict(f_lo=0.0), "f_lo nan": dict(f_lo=np.nan), "f_lo inf": dict(f_lo=np.inf),
           "dv 0": dict(dv=0.0), "dv nan": dict(dv=np.nan), "dv inf": dict(dv=np.inf), "dv < 0": dict(dv=-0.1),
           "T = W": dict(T=Wd.ptr), "T inside dW": dict(T=dWd.ptr + (rows - 1) * ld * cs), "T ends in W": dict(T=Wd.ptr - (nf - 1) * ld * cs - cs)}
    out = []
    for label, change in bad.items():
        a = dict(good, **change)
        rc = lib.cwt_ssq_reassign(h, P(a["W"]), P(a["dW"]), a["ld"], a["ncols"], a["nrows"], a["w"], a["gamma"], a["f_lo"], a["dv"],
                                  a["nf"], P(a["T"]), a["ldt"], 0)
        out.append((label, rc))
    for label, (x, dt, y) in {"xhat NULL": (None, 1.0, Td.ptr), "yhat NULL": (Td.ptr, 1.0, None), "dt 0": (Td.ptr, 0.0, Td.ptr),
                              "dt nan": (Td.ptr, np.nan, Td.ptr)}.items():
        out.append((label, lib.cwt_spectrum_derivative(h, P(x), dt, P(y))))
    out.append(("plan NULL", lib.cwt_ssq_reassign(None, P(Wd.ptr), P(dWd.ptr), ld, ncols, rows, wp, GAMMA, F_LO, DV, nf, P(Td.ptr), ld, 0)))
    dev.plan.sync()
    untouched = all(np.array_equal(b.download(dev.plan, a.shape, dev.cplx), a, equal_nan=True)
                    for b, a in ((Td, start), (Wd, padded(W, 3, 0)), (dWd, padded(dW, 3, 0))))
    dev.release()
    return out, untouched


# ---- cwt_spectrum_derivative ------------------------------------------------------------------------------------------------------
def check_spectrum_derivative(dev, N, dt=0.25):
    """against long double: 8 eps per bin (w_k in double: three roundings; the product: one; well inside), Nyquist exactly 0, in
    place = out of place"""
    assert dev.plan.nfft == N
    rng = np.random.default_rng(N)
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(dev.cplx)
    xd, yd = dev.up(x), dev.up(np.full(N, SENTINEL, dtype=dev.cplx))
    dev.plan.spectrum_derivative(xd.ptr, dt, yd.ptr)
    y = yd.download(dev.plan, (N,), dev.cplx)
    assert np.array_equal(xd.download(dev.plan, (N,), dev.cplx), x)
    dev.plan.spectrum_derivative(xd.ptr, dt, xd.ptr)
    assert np.array_equal(xd.download(dev.plan, (N,), dev.cplx).view(dev.real), y.view(dev.real))
    sk = np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(L)
    wk = 2 * L(np.pi) * sk / (L(N) * L(dt))
    wk[N // 2] = 0
    ref_re, ref_im = -wk * x.imag.astype(L), wk * x.real.astype(L)
    err = np.hypot(y.real.astype(L) - ref_re, y.imag.astype(L) - ref_im)
    assert (err <= 8 * L(dev.eps) * np.hypot(ref_re, ref_im)).all(), float((err / np.hypot(ref_re, ref_im)[err > 0]).max() if (err > 0).any() else 0)
    assert y[N // 2] == 0
    dev.release()


def check_derivative_rows(dev, mother, n0, rows, tol):
    """dW rows = cwt_transform_rows of the derivative spectrum against ifft(i w xhat F_j) of the oracle: the error of a row
    relative to its peak within the round-off tolerance tests/test_gpu_parity.py holds W to"""
    kind, param = MOTHERS[mother]
    m = orc.Mother(kind, param)
    N, dt = dev.plan.nfft, 0.5
    s0 = 2 * dt / m.flambda()
    sj = s0 * 2 ** (np.arange(rows) * np.log2(n0 * dt / s0) / max(rows - 1, 1))
    sj = sj[~orc.dropped_rows(sj, dt, m)]
    x = np.random.default_rng(n0).standard_normal(n0).astype(dev.real)
    xd, xh = dev.up(x), dev.up(np.zeros(N, dtype=dev.cplx))
    dWd = dev.up(np.zeros((sj.size, n0), dtype=dev.cplx))
    dev.plan.forward_fft(xd.ptr, n0, xh.ptr)
    dev.plan.spectrum_derivative(xh.ptr, dt, xh.ptr)
    dev.plan.transform_rows(xh.ptr, kind, param, dt, sj, dWd.ptr, n0, n0)
    dW = dWd.download(dev.plan, (sj.size, n0), dev.cplx)
    dev.release()
    ref = derivative_rows_oracle(x.astype(np.float64), dt, sj, m, N)[:, :n0]
    per_row = np.abs(dW - ref).max(axis=1) / np.abs(ref).max(axis=1)
    assert per_row.max() < tol, (int(per_row.argmax()), float(per_row.max()))


def derivative_rows_oracle(x, dt, sj, m, N):
    """ifft(i w xhat F_j): the oracle's rows of the signal whose spectrum is i w xhat (Nyquist bin 0) -- its own transform of that
    real signal"""
    xhat = np.fft.fft(x, n=N)
    w = 2 * np.pi * np.fft.fftfreq(N, dt)
    w[N // 2] = 0
    xdot = np.fft.ifft(1j * w * xhat).real
    return orc.cwt_rows(xdot, dt, sj, m, N=N)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def plan_w_dw(H):
    """W and dW of a DeviceSynchrosqueezed in the plan's precision (the bits the reassignment saw)"""
    plan = H._plan
    return H.W().astype(plan.cplx), H.dW().astype(plan.cplx)


def tone(N, dj, mother_name, prec):
    """(x, k0, dt, bin): cos(2 pi k0 n / N + phi) on an FFT bin whose frequency lies within 0.05 bin of a centre of the default grid.
    k0 / N in [1/16, 1/4]: the reference's Morlet filter is not cut at f = 0, so a row sees the tone's negative line too, B / A =
    exp(-2 f0 s w0) of the positive one; that ratio wiggles the instantaneous frequency by 2 (B / A) / (ln 2 dj) bins.  At the
    smallest scale (s0 = 1.94 dt) and w0 >= 2 pi / 16 it is below 1e-4, 0.004 bin at dj = 1 / 12; at larger scales smaller still."""
    import pycwt_amd
    dt = 1.0
    mother = pycwt_amd.wavelet._check_parameter_wavelet(mother_name)
    _, sj, freqs, _, _, bad = pycwt_amd.wavelet._geometry(mother, N, dt, dj, -1, -1, None, True)
    freqs = np.asarray(freqs)[~bad] if bad is not None else np.asarray(freqs)
    f_lo = freqs.min()
    best = None
    for k0 in range(N // 16, N // 4):
        pos = np.log2(k0 / (N * dt) / f_lo) / dj
        d = abs(pos - np.round(pos))
        if d < 0.05 and (best is None or d < best[1]):
            best = (k0, d)
    k0 = best[0]
    x = np.cos(2 * np.pi * k0 * np.arange(N) / N + 0.7)
    return x, k0, dt, int(np.round(np.log2(k0 / (N * dt) / f_lo) / dj))


def check_tone(N, mother_name, prec, dj=1 / 12):
    """every cell outside the tone's bin exactly 0; the bin's row = the long-double sum of the plan's own W / sqrt(s_j) over the
    entries above gamma"""
    import pycwt_amd
    real, cplx, eps = types(prec)
    x, k0, dt, kbin = tone(N, dj, mother_name, prec)
    H = pycwt_amd.ssq_cwt_device(x, dt, dj, wavelet=mother_name, precision=prec)
    try:
        T, W = H.T().astype(cplx), H.W().astype(cplx)
        gamma = float(np.sqrt(eps) * np.std(x))
        w = 1.0 / np.sqrt(H.sj)
        assert 0 < kbin < H.ssq_freqs.size - 1
        off = np.delete(T, kbin, axis=0)
        assert np.all(off == 0), (int((off != 0).sum()), np.argwhere(np.delete(T, kbin, axis=0) != 0)[:4].tolist())
        with np.errstate(all="ignore"):
            a2 = W.real * W.real + W.imag * W.imag
        above = a2.astype(np.float64) > gamma * gamma
        wl = w.astype(L)[:, None]
        ref_re = (wl * np.where(above, W.real, 0).astype(L)).sum(axis=0)
        ref_im = (wl * np.where(above, W.imag, 0).astype(L)).sum(axis=0)
        mag = (wl * np.where(above, np.abs(W), 0).astype(L)).sum(axis=0)
        m = above.sum(axis=0)
        assert m.min() >= 1
        err = np.hypot(T[kbin].real.astype(L) - ref_re, T[kbin].imag.astype(L) - ref_im)
        assert (err <= (m + 3) * L(eps) * mag).all(), float((err / ((m + 3) * L(eps) * mag)).max())
    finally:
        H.close()


def chirp_in_noise(n0, seed):
    """white noise (std 0.1) plus a unit chirp from 0.02 to 0.1 cycles per sample; returns (x, chirp)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n0)
    phase = 2 * np.pi * (0.02 * t + 0.5 * (0.08 / n0) * t * t)
    c = np.cos(phase)
    return c + 0.1 * rng.standard_normal(n0), c


def check_noise_chirp(n0, prec, dj, seed, mother_name="morlet", full_reference=True):
    """the column-sum invariant; gamma = 0 on a widened grid: issq = icwt; the band around the chirp's ridge gives the chirp back
    closer than its complement does; fp64: T against the reference built from the plan's own W and dW"""
    import pycwt_amd
    real, cplx, eps = types(prec)
    x, c = chirp_in_noise(n0, seed)
    dt = 1.0
    out = {}
    H = pycwt_amd.ssq_cwt_device(x, dt, dj, wavelet=mother_name, precision=prec)
    try:
        T = H.T().astype(cplx)
        W, dW = plan_w_dw(H)
        gamma = float(np.sqrt(eps) * np.std(x))
        f_lo, nf = float(H.ssq_freqs[0]), H.ssq_freqs.size
        assert np.array_equal(np.asarray(H.ssq_freqs), f_lo * 2.0 ** (dj * np.arange(nf)))
        ref = Reference(W, dW, 1.0 / np.sqrt(H.sj), gamma, f_lo, dj, nf)
        out["dropped"] = 1 - ref.kept.mean()
        assert_column_sums(T, ref, eps)
        if prec == 64 and full_reference:
            doubt = ref.doubtful_cells()
            out["left_out"] = doubt.mean()
            assert doubt.mean() <= 1e-3, doubt.mean()
            assert_cells(T, ref, eps, where=~doubt)
            assert np.all(T[(ref.m == 0) & ~doubt] == 0)
        # a band of +- half an octave around the ridge 0.02 ... 0.1: the chirp, against everything else
        band = (0.02 / 2 ** 0.5, 0.1 * 2 ** 0.5)
        inside, total = H.issq(dj, band=band), H.issq(dj)
        outside = total - inside
        core = slice(n0 // 8, n0 - n0 // 8)                        # (away from the edges, where the zero padding bends the ridge)
        e_in, e_out = np.abs(inside.real - c)[core], np.abs(outside.real - c)[core]
        out["band_rms"] = (np.sqrt((e_in ** 2).mean()), np.sqrt((e_out ** 2).mean()))
        assert out["band_rms"][0] < out["band_rms"][1]
        host = pycwt_amd.issq_cwt(T, dt, dj, mother_name, ssq_freqs=np.asarray(H.ssq_freqs), band=band, precision=prec)
        np.testing.assert_allclose(host, inside, rtol=0, atol=nf * eps * np.abs(inside).max())
    finally:
        H.close()
    # gamma = 0 and a grid of three octaves more on either side: nothing with q > 0 falls outside, the column sum is the icwt sum
    wide = (f_lo / 8, dj, nf + int(round(6 / dj)))
    H0 = pycwt_amd.ssq_cwt_device(x, dt, dj, wavelet=mother_name, precision=prec, gamma=0.0, ssq_freqs=wide)
    D = pycwt_amd.cwt_device(x, dt, dj, wavelet=mother_name, precision=prec)
    try:
        W, dW = plan_w_dw(H0)
        ref0 = Reference(W, dW, 1.0 / np.sqrt(H0.sj), 0.0, wide[0], dj, wide[2])
        rows = H0.sj.size
        a, b = H0.issq(dj), D.icwt(dj)
        # entries with q <= 0 (or outside even this grid) are in icwt's sum and not in issq's: the reference says which
        coeff = dj * np.sqrt(dt) / (H0.mother.cdelta * H0.mother.psi(0))
        wl = (1.0 / np.sqrt(H0.sj)).astype(L)[:, None]
        missing = (wl * np.where(ref0.kept, 0, np.nan_to_num(W.real)).astype(L)).sum(axis=0).astype(np.float64)
        scale = (wl * np.abs(W).astype(L)).sum(axis=0).astype(np.float64)
        out["dropped_wide"] = 1 - ref0.kept.mean()
        err = np.abs(a - (b - coeff * missing)) / abs(coeff)
        assert (err <= rows * eps * scale).all(), float((err / (eps * scale)).max())
    finally:
        H0.close()
        D.close()
    return out
