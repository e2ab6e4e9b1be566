"""Shared by tests/test_ssq_grad_emulated.py, tests/test_ssq_grad_schedules_emulated.py and tests/test_ssq_grad_gpu.py: the cases of
the differentiable synchrosqueezed transform -- cwt_ssq_reassign_bins, cwt_ssq_gather (include/cwt_hip.h) and the torch entry
points ssq_cwt_torch / issq_cwt_torch around them -- built on the definition restated in tests/ssq_common.py.

Export level: T of cwt_ssq_reassign_bins is cwt_ssq_reassign's bit for bit and its map is `decisions()`' k (-1 where an entry is
not kept); cwt_ssq_gather is its NumPy restatement bit for bit (w rounded to T, one product per component, +0 by selection); the
pair is a transpose pair within the counting of `Reference.bound`.  Torch level: the saved map and Tx against `Reference` on the
engine's own W and dW; x.grad bit for bit through cwt_torch's backward on the cotangent gathered on the host; and an
independent finite difference at a point where the map does not move, so that T is exactly linear along the step.
"""
import ctypes as C

import numpy as np

import ssq_common as sc
from ssq_common import DV, EINVAL, F_LO, GAMMA, L, SENTINEL  # noqa: F401

ROWS, NCOLS, NFS = (1, 7, 8, 9, 13, 24), (1, 127, 128, 129, 300), (1, 5)      # around the 8 rows in flight / the 128-thread workgroup
BIG_NF = (32767, 3)                                                           # (nf, ncols): the largest grid the int16 map holds
FINE_DV = 2.0 ** -12                                                          # 32767 bins of 1 / 12 octave would leave double's range
BIN_SENTINEL = -77
PAD = 3


def planted(seed, rows, ncols, nf, prec):
    """(W, dW, w, ref, dv): ssq_common.synthetic (every kind of dropped entry, runs of equal bins), or for a grid too long for it
    the same idea on a fine grid: entries on bins 0, 1, nf - 2, nf - 1 and random ones, 0.25 bin from every edge, every fifth entry
    just outside the grid (-1 or nf)"""
    if nf * DV < 900:
        return sc.synthetic(seed, rows, ncols, nf, prec) + (DV,)
    real, cplx, eps = sc.types(prec)
    rng = np.random.default_rng(seed)
    tk = rng.choice([0, 1, nf - 2, nf - 1, int(rng.integers(2, nf - 2))], size=(rows, ncols))
    flat = np.arange(rows * ncols).reshape(rows, ncols)
    tk = np.where(flat % 5 == 2, -1, np.where(flat % 5 == 4, nf, tk))
    f = F_LO * 2.0 ** ((tk + rng.uniform(-0.25, 0.25, size=tk.shape)) * FINE_DV)
    W = (GAMMA * rng.uniform(2.0, 10.0, size=tk.shape) * np.exp(2j * np.pi * rng.random(tk.shape))).astype(cplx)
    dW = (2j * np.pi * f * W.astype(np.complex128)).astype(cplx)
    w = rng.uniform(0.2, 2.0, size=rows)
    ref = sc.Reference(W, dW, w, GAMMA, F_LO, FINE_DV, nf)
    assert np.array_equal(ref.kept, (tk >= 0) & (tk < nf)) and np.array_equal(ref.k[ref.kept], tk[ref.kept])     # the construction
    return W, dW, w, ref, FINE_DV


def expected_bins(ref):
    return np.where(ref.kept, ref.k, -1).astype(np.int16)


def run_reassign_bins(dev, W, dW, w, nf, dv=DV, chunks=None, T0=None):
    """cwt_ssq_reassign_bins over the rows in chunks (None: one call); ld = ldt = ldb = ncols + PAD, the padding of T and bins
    holding sentinels.  Returns (T, bins) with their padding."""
    rows, ncols = W.shape
    ld = ncols + PAD
    nan = complex(np.nan, np.nan)
    Wd, dWd = dev.up(sc.padded(W, PAD, nan)), dev.up(sc.padded(dW, PAD, nan))
    start = np.full((nf, ld), SENTINEL, dtype=dev.cplx)
    if T0 is not None:
        start[:, :ncols] = T0
    Td, Bd = dev.up(start), dev.up(np.full((rows, ld), BIN_SENTINEL, dtype=np.int16))
    cs = np.dtype(dev.cplx).itemsize
    step = chunks or rows
    for a in range(0, rows, step):
        b = min(rows, a + step)
        dev.plan.ssq_reassign_bins(Wd.ptr + a * ld * cs, dWd.ptr + a * ld * cs, ld, ncols, w[a:b], GAMMA, F_LO, dv, nf, Td.ptr, ld,
                                   T0 is not None or a > 0, Bd.ptr + a * ld * 2, ld)
    T, bins = Td.download(dev.plan, (nf, ld), dev.cplx), Bd.download(dev.plan, (rows, ld), np.int16)
    dev.release()
    return T, bins


def run_reassign(dev, W, dW, w, nf, dv=DV, chunks=None):
    return sc.run_reassign(dev, W, dW, w, nf, dv=dv, pad=PAD, chunks=chunks)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_reassign_bins(dev, rows, ncols, nf, chunkings=(None,)):
    """T bit for bit cwt_ssq_reassign's, bins = the decisions of the definition, sentinels intact; for every way of chunking the
    rows.  Returns (W, dW, w, ref, dv, T, bins) of the case."""
    W, dW, w, ref, dv = planted(1000 * rows + 10 * (nf % 997) + ncols, rows, ncols, nf, dev.prec)
    want_T = run_reassign(dev, W, dW, w, nf, dv)
    assert np.all(want_T[:, ncols:] == SENTINEL)
    for chunks in chunkings:
        T, bins = run_reassign_bins(dev, W, dW, w, nf, dv, chunks)
        assert same_bits(T, want_T), chunks
        assert bins.dtype == np.int16 and np.array_equal(bins[:, :ncols], expected_bins(ref)), chunks
        assert np.all(bins[:, ncols:] == BIN_SENTINEL), chunks
    return W, dW, w, ref, dv, T[:, :ncols], bins[:, :ncols]


def check_accumulate_adds(dev, rows=13, ncols=129, nf=5):
    """accumulate = 1 on a T that holds something: the bits of cwt_ssq_reassign on the same T, the same map"""
    W, dW, w, ref, dv = planted(78, rows, ncols, nf, dev.prec)
    rng = np.random.default_rng(6)
    T0 = (rng.standard_normal((nf, ncols)) + 1j * rng.standard_normal((nf, ncols))).astype(dev.cplx)
    want = sc.run_reassign(dev, W, dW, w, nf, pad=PAD, T0=T0)
    T, bins = run_reassign_bins(dev, W, dW, w, nf, T0=T0)
    assert same_bits(T, want) and np.array_equal(bins[:, :ncols], expected_bins(ref))


def reassign_bins_refusals(dev, rows=8, ncols=127, nf=5):
    """(label, return code) of every argument set cwt_ssq_reassign_bins refuses -- what cwt_ssq_reassign refuses and its own --
    and whether T, bins, W and dW are as they were"""
    W, dW, w, _, _ = planted(3, rows, ncols, nf, dev.prec)
    ld = ncols + PAD
    cs = np.dtype(dev.cplx).itemsize
    Wd, dWd = dev.up(sc.padded(W, PAD, 0)), dev.up(sc.padded(dW, PAD, 0))
    start, bstart = np.full((max(nf, rows), ld), SENTINEL, dtype=dev.cplx), np.full((rows + 2, ld), BIN_SENTINEL, dtype=np.int16)
    Td, Bd = dev.up(start), dev.up(bstart)
    lib, h, P = dev.lib, dev.plan.h, C.c_void_p
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(W=Wd.ptr, dW=dWd.ptr, ld=ld, ncols=ncols, nrows=rows, w=wp, gamma=GAMMA, f_lo=F_LO, dv=DV, nf=nf, T=Td.ptr, ldt=ld,
                bins=Bd.ptr, ldb=ld)
    bins_bytes = ((rows - 1) * ld + ncols) * 2
    bad = {"W NULL": dict(W=None), "dW NULL": dict(dW=None), "T NULL": dict(T=None), "weights NULL": dict(w=None),
           "bins NULL": dict(bins=None), "nrows 0": dict(nrows=0), "nrows > max_rows": dict(nrows=dev.plan.max_rows + 1),
           "ncols 0": dict(ncols=0), "ld < ncols": dict(ld=ncols - 1), "ldt < ncols": dict(ldt=ncols - 1), "ldb < ncols": dict(ldb=ncols - 1),
           "nf 0": dict(nf=0), "nf 32768": dict(nf=32768), "gamma nan": dict(gamma=np.nan), "gamma inf": dict(gamma=np.inf),
           "gamma < 0": dict(gamma=-1.0), "f_lo 0": dict(f_lo=0.0), "f_lo nan": dict(f_lo=np.nan), "f_lo inf": dict(f_lo=np.inf),
           "dv 0": dict(dv=0.0), "dv nan": dict(dv=np.nan), "dv inf": dict(dv=np.inf), "dv < 0": dict(dv=-0.1),
           "T = W": dict(T=Wd.ptr), "T inside dW": dict(T=dWd.ptr + (rows - 1) * ld * cs),
           "bins = W": dict(bins=Wd.ptr), "bins inside dW": dict(bins=dWd.ptr + (rows - 1) * ld * cs), "bins = T": dict(bins=Td.ptr),
           "bins ends in T": dict(bins=Td.ptr - bins_bytes + 2), "bins starts in T's last element": dict(bins=Td.ptr + ((nf - 1) * ld + ncols) * cs - 2)}
    out = []
    for label, change in bad.items():
        a = dict(good, **change)
        rc = lib.cwt_ssq_reassign_bins(h, P(a["W"]), P(a["dW"]), a["ld"], a["ncols"], a["nrows"], a["w"], a["gamma"], a["f_lo"], a["dv"],
                                       a["nf"], P(a["T"]), a["ldt"], 0, P(a["bins"]), a["ldb"])
        out.append((label, rc))
    out.append(("plan NULL", lib.cwt_ssq_reassign_bins(None, P(Wd.ptr), P(dWd.ptr), ld, ncols, rows, wp, GAMMA, F_LO, DV, nf, P(Td.ptr), ld, 0,
                                                       P(Bd.ptr), ld)))
    dev.plan.sync()
    untouched = (np.array_equal(Td.download(dev.plan, start.shape, dev.cplx), start)
                 and np.array_equal(Bd.download(dev.plan, bstart.shape, np.int16), bstart)
                 and np.array_equal(Wd.download(dev.plan, (rows, ld), dev.cplx), sc.padded(W, PAD, 0), equal_nan=True)
                 and np.array_equal(dWd.download(dev.plan, (rows, ld), dev.cplx), sc.padded(dW, PAD, 0), equal_nan=True))
    dev.release()
    return out, untouched


# ---- cwt_ssq_gather --------------------------------------------------------------------------------------------------------------
def gather_reference(gT, bins, w, real):
    """the definition: w rounded to T, one product per component in T (NumPy's arithmetic of that type), +0 by selection"""
    nf = gT.shape[0]
    ok = (bins >= 0) & (bins < nf)
    k = np.where(ok, bins, 0).astype(np.int64)
    cols = np.broadcast_to(np.arange(bins.shape[1]), bins.shape)
    wT = np.asarray(w, dtype=np.float64).astype(real)[:, None]
    with np.errstate(all="ignore"):
        re, im = wT * gT.real[k, cols], wT * gT.imag[k, cols]
    G = np.zeros(bins.shape, dtype=gT.dtype)
    G.real[ok], G.imag[ok] = re[ok], im[ok]
    return G, ok


def run_gather(dev, gT, bins, w, guard=1):
    """cwt_ssq_gather with ldt = ldb = ldg = ncols + PAD into a G that has `guard` rows of sentinels before and after it.
    Returns G with its padding and the guard rows."""
    rows, ncols = bins.shape
    nf, ld = gT.shape[0], ncols + PAD
    cs = np.dtype(dev.cplx).itemsize
    Td, Bd = dev.up(sc.padded(gT, PAD, complex(np.nan, np.nan))), dev.up(sc.padded(bins, PAD, 0))
    Gd = dev.up(np.full((rows + 2 * guard, ld), SENTINEL, dtype=dev.cplx))
    dev.plan.ssq_gather(Td.ptr, ld, nf, Bd.ptr, ld, w, ncols, Gd.ptr + guard * ld * cs, ld)
    G = Gd.download(dev.plan, (rows + 2 * guard, ld), dev.cplx)
    assert np.array_equal(Bd.download(dev.plan, (rows, ld), np.int16), sc.padded(bins, PAD, 0))                 # inputs are inputs
    dev.release()
    return G, guard


def assert_gather(G_all, guard, gT, bins, w, real):
    rows, ncols = bins.shape
    assert np.all(G_all[:guard] == SENTINEL) and np.all(G_all[guard + rows:] == SENTINEL) and np.all(G_all[:, ncols:] == SENTINEL)
    G = G_all[guard:guard + rows, :ncols]
    want, ok = gather_reference(gT, bins, w, real)
    nan = np.isnan(want.real) | np.isnan(want.imag)
    assert np.array_equal(np.isnan(G.real), np.isnan(want.real)) and np.array_equal(np.isnan(G.imag), np.isnan(want.imag))
    assert same_bits(np.where(np.isnan(G.real), 0, G.real), np.where(np.isnan(want.real), 0, want.real))
    assert same_bits(np.where(np.isnan(G.imag), 0, G.imag), np.where(np.isnan(want.imag), 0, want.imag))
    assert not nan[~ok].any()
    assert np.all(G[~ok] == 0) and not np.signbit(G.real[~ok]).any() and not np.signbit(G.imag[~ok]).any()         # exactly +0
    return G


def gather_inputs(seed, bins, nf, prec, poison=True):
    """(gT, bins, w) for a map: random gT; with `poison`, NaN and Inf in the cells no entry of their column points to, the last
    column (of more than one) all dropped with NaN in its row 0, one pointed-to cell NaN, and planted bins >= nf and < -1"""
    real, cplx, eps = sc.types(prec)
    rng = np.random.default_rng(seed)
    rows, ncols = bins.shape
    bins = bins.copy()
    gT = (rng.standard_normal((nf, ncols)) + 1j * rng.standard_normal((nf, ncols))).astype(cplx)
    w = rng.uniform(0.2, 2.0, size=rows)
    if not poison:
        return gT, bins, w
    if ncols > 1:
        bins[:, -1] = -1
    flat = np.arange(rows * ncols).reshape(rows, ncols)
    bins[(flat % 29 == 5) & (bins >= 0)] = nf                             # a caller's error: dropped, nothing read
    bins[flat % 31 == 7] = 32767
    bins[flat % 37 == 9] = -32768
    used = np.zeros((nf, ncols), dtype=bool)
    ok = (bins >= 0) & (bins < nf)
    used[bins[ok], np.broadcast_to(np.arange(ncols), bins.shape)[ok]] = True
    free = np.argwhere(~used)
    for i, (k, n) in enumerate(free):
        gT[k, n] = (complex(np.nan, 1.0), complex(np.inf, -np.inf), complex(2.0, np.nan))[i % 3]
    if ncols > 1:
        assert not used[:, -1].any()
        gT[0, -1] = complex(np.nan, np.nan)
    hit = np.argwhere(used)
    if len(hit):
        gT[tuple(hit[len(hit) // 2])] = complex(np.nan, np.inf)              # reaches the entries of that cell, and only those
    return gT, bins, w


def check_gather(dev, rows, ncols, nf):
    ref = planted(7000 + 100 * rows + 10 * (nf % 997) + ncols, rows, ncols, nf, dev.prec)[3]
    gT, bins, w = gather_inputs(rows + ncols + nf, expected_bins(ref), nf, dev.prec)
    G_all, guard = run_gather(dev, gT, bins, w)
    return assert_gather(G_all, guard, gT, bins, w, dev.real)


def gather_refusals(dev, rows=8, ncols=127, nf=5):
    ref = planted(4, rows, ncols, nf, dev.prec)[3]
    gT, bins, w = gather_inputs(9, expected_bins(ref), nf, dev.prec, poison=False)
    ld = ncols + PAD
    cs = np.dtype(dev.cplx).itemsize
    Td, Bd = dev.up(sc.padded(gT, PAD, 0)), dev.up(sc.padded(bins, PAD, 0))
    gstart = np.full((max(rows, nf) + 2, ld), SENTINEL, dtype=dev.cplx)
    Gd = dev.up(gstart)
    lib, h, P = dev.lib, dev.plan.h, C.c_void_p
    wp = w.ctypes.data_as(C.POINTER(C.c_double))
    good = dict(gT=Td.ptr, ldt=ld, nf=nf, bins=Bd.ptr, ldb=ld, w=wp, nrows=rows, ncols=ncols, G=Gd.ptr, ldg=ld)
    g_bytes = ((rows - 1) * ld + ncols) * cs
    bad = {"gT NULL": dict(gT=None), "bins NULL": dict(bins=None), "weights NULL": dict(w=None), "G NULL": dict(G=None),
           "nrows 0": dict(nrows=0), "nrows > max_rows": dict(nrows=dev.plan.max_rows + 1), "ncols 0": dict(ncols=0), "nf 0": dict(nf=0),
           "nf 32768": dict(nf=32768), "ldt < ncols": dict(ldt=ncols - 1), "ldb < ncols": dict(ldb=ncols - 1), "ldg < ncols": dict(ldg=ncols - 1),
           "G = gT": dict(G=Td.ptr), "G = bins": dict(G=Bd.ptr), "G ends in gT": dict(G=Td.ptr - g_bytes + cs),
           "G starts in the last element of bins": dict(G=Bd.ptr + ((rows - 1) * ld + ncols) * 2 - 2)}
    out = []
    for label, change in bad.items():
        a = dict(good, **change)
        out.append((label, lib.cwt_ssq_gather(h, P(a["gT"]), a["ldt"], a["nf"], P(a["bins"]), a["ldb"], a["w"], a["nrows"], a["ncols"],
                                              P(a["G"]), a["ldg"])))
    out.append(("plan NULL", lib.cwt_ssq_gather(None, P(Td.ptr), ld, nf, P(Bd.ptr), ld, wp, rows, ncols, P(Gd.ptr), ld)))
    dev.plan.sync()
    untouched = (np.array_equal(Gd.download(dev.plan, gstart.shape, dev.cplx), gstart)
                 and np.array_equal(Td.download(dev.plan, (nf, ld), dev.cplx), sc.padded(gT, PAD, 0))
                 and np.array_equal(Bd.download(dev.plan, (rows, ld), np.int16), sc.padded(bins, PAD, 0)))
    dev.release()
    return out, untouched


# ---- the pair is a transpose pair --------------------------------------------------------------------------------------------------
def check_transpose(dev, rows, ncols, nf):
    """Re sum conj(gT) T = Re sum conj(G) W over the kept entries (a dropped entry of W may be NaN; its G is +0 and it takes no part),
    both sums in long double.  T's cell carries (m + 3) eps sum |w_j W| (Reference.bound); G's element one product and the weight's
    rounding, which that count already holds.  So the bound is sum over the cells of |gT| (m + 3) eps sum |w_j W|."""
    W, dW, w, ref, dv, T, bins = check_reassign_bins(dev, rows, ncols, nf)
    gT, bins, w2 = gather_inputs(5 * rows + ncols, bins, nf, dev.prec, poison=False)
    G_all, guard = run_gather(dev, gT, bins, w)
    G = assert_gather(G_all, guard, gT, bins, w, dev.real)
    def redot(a, b, where=None):
        t = a.real.astype(L) * b.real.astype(L) + a.imag.astype(L) * b.imag.astype(L)
        return t.sum() if where is None else t[where].sum()
    lhs, rhs = redot(gT, T), redot(G, W, ref.kept)
    bound = (np.abs(gT).astype(L) * ref.bound(dev.eps)).sum()
    assert abs(lhs - rhs) <= bound, (float(lhs), float(rhs), float(bound))


# ---- schedules ---------------------------------------------------------------------------------------------------------------------
GRAD_KERNELS = {"ssqg_reassign_bins", "ssqg_gather"}


def schedule_case(lib, prec):
    """a reassignment with bins of 13 x 300 entries in two row chunks, and a gather through that map over 13 rows (two stretches of
    rows per column): every kernel of cwt_kernels_ssq_grad.hpp, as bytes"""
    with sc.Dev(lib, 16, prec, max_rows=16) as dev:
        W, dW, w, ref, dv = planted(21, 13, 300, 5, prec)
        T, bins = run_reassign_bins(dev, W, dW, w, 5, chunks=8)
        gT, b2, w2 = gather_inputs(2, bins[:, :300], 5, prec)
        G, _ = run_gather(dev, gT, b2, w2)
    return np.concatenate([T.view(np.uint8).ravel(), bins.view(np.uint8).ravel(), G.view(np.uint8).ravel()])


# ---- torch -------------------------------------------------------------------------------------------------------------------------
TORCH_MOTHERS = {"morlet": 6, "paul": 4}


def engine_of(x, n0):
    """the engine the torch entry points used for x"""
    from pycwt_amd import autograd
    prec = 64 if str(x.dtype).endswith("64") else 32
    N = 1 << int(np.ceil(np.log2(n0)))
    found = [e for key, e in autograd._engines.items() if key[0] == N and key[1] == prec]
    assert len(found) == 1
    return found[0]


def signal(n0, seed, prec):
    """noise plus a chirp, in the precision of the case"""
    return sc.chirp_in_noise(n0, seed)[0].astype(sc.types(prec)[0])


def host_gamma(x, prec):
    return float(np.sqrt(sc.types(prec)[2]) * np.std(np.asarray(x, dtype=np.float64)))


def engine_w_dw(torch, xt, dt, dj, name):
    """W = cwt_torch(x) and the dW that plan.spectrum_derivative + transform_rows give on the same engine, one signal; as NumPy"""
    import pycwt_amd
    n0 = xt.shape[-1]
    W, sj = pycwt_amd.cwt_torch(xt, dt, dj, wavelet=name)[:2]
    eng = engine_of(xt, n0)
    kind, param = sc.MOTHERS[name]
    xhat = torch.empty(eng.plan.nfft, dtype=W.dtype, device=xt.device)
    dW = torch.empty_like(W)
    eng.forward(xt, n0, xhat)
    eng.plan.spectrum_derivative(xhat.data_ptr(), dt, xhat.data_ptr())
    eng.plan.transform_rows(xhat.data_ptr(), kind, float(param), dt, sj, dW.data_ptr(), n0, n0)
    return W, dW, sj


def check_torch_forward(torch, device, n0, name, prec, batch, dj=1 / 4, seed=31):
    """one chunk: the saved map = decisions(W, dW), Tx within Reference's bound in every cell; chunks of 5 rows: within the bound
    outside the doubtful cells, at most 1 % of the non-empty ones; the grids are ssq_cwt's; a batch row has the bits of its signal
    alone"""
    import pycwt_amd
    from pycwt_amd import autograd, wavelet
    real, cplx, eps = sc.types(prec)
    dt = 0.5
    xs = np.stack([signal(n0, seed + b, prec) for b in range(batch or 1)])
    xt = torch.tensor(xs if batch else xs[0], device=device, requires_grad=True)
    keep = wavelet.SSQ_CHUNK_ROWS
    try:
        wavelet.SSQ_CHUNK_ROWS = 1 << 20
        Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt_torch(xt, dt, dj, wavelet=name)
        bins = autograd._ssq_saved_bins(Tx)
        wavelet.SSQ_CHUNK_ROWS = 5
        Tx5 = pycwt_amd.ssq_cwt_torch(xt, dt, dj, wavelet=name)[0]
    finally:
        wavelet.SSQ_CHUNK_ROWS = keep
    nf = fs.size
    assert Tx.shape == xt.shape[:-1] + (nf, n0) and Tx.dtype == (torch.complex128 if prec == 64 else torch.complex64)
    assert Tx.device == xt.device and bins.dtype == torch.int16 and bins.shape == xt.shape[:-1] + (sj.size, n0)
    want = pycwt_amd.ssq_cwt(xs[0].astype(np.float64), dt, dj, wavelet=name, precision=prec)
    for got, ref in zip((fs, sj, freqs, coi), want[1:]):
        assert np.array_equal(got, ref)
    f_lo = float(fs[0])
    for b in range(batch or 1):
        xb = xt.detach()[b] if batch else xt.detach()
        Tb, T5b, bb = (t[b] if batch else t for t in (Tx.detach(), Tx5.detach(), bins))
        if batch:
            xb1 = xb.clone().requires_grad_(True)
            alone = pycwt_amd.ssq_cwt_torch(xb1, dt, dj, wavelet=name)[0]
            assert torch.equal(alone.detach(), Tb) or same_bits(alone.detach().cpu().numpy(), Tb.cpu().numpy())
            assert torch.equal(autograd._ssq_saved_bins(alone), bb)
        W, dW, sj2 = engine_w_dw(torch, xb, dt, dj, name)
        assert np.array_equal(sj2, sj)
        Wn, dWn, gamma = W.cpu().numpy(), dW.cpu().numpy(), host_gamma(xs[b], prec)
        if batch and n0 > 4096 and b < batch - 1:          # (the long-double sums of a long signal take seconds: the map of every
            kept, k = sc.decisions(Wn, dWn, gamma, f_lo, dj, nf)[:2]      # signal, the sums of the last one -- each has the bits of
            assert np.array_equal(bb.cpu().numpy(), np.where(kept, k, -1))          # its signal alone, asserted above)
            continue
        ref = sc.Reference(Wn, dWn, 1.0 / np.sqrt(sj), gamma, f_lo, dj, nf)
        assert np.array_equal(bb.cpu().numpy(), expected_bins(ref))
        T = Tb.cpu().numpy()
        sc.assert_cells(T, ref, eps)
        assert np.all(T[ref.m == 0] == 0)
        doubt = ref.doubtful_cells()
        assert doubt.sum() <= 0.01 * (ref.m > 0).sum(), (int(doubt.sum()), int((ref.m > 0).sum()))
        sc.assert_cells(T5b.cpu().numpy(), ref, eps, where=~doubt)


def check_torch_refusals(torch, device):
    import pycwt_amd
    import pytest
    x = torch.tensor(signal(128, 3, 64), device=device)

    class Duck:
        def psi_ft(self, f):
            return pycwt_amd.Morlet(6).psi_ft(f)

        def flambda(self):
            return pycwt_amd.Morlet(6).flambda()

        def coi(self):
            return pycwt_amd.Morlet(6).coi()
    for kw in (dict(wavelet="dog"), dict(wavelet="mexicanhat"), dict(wavelet=pycwt_amd.DOG(3)), dict(wavelet=Duck()),
               dict(freqs=np.array([0.1, 0.2])), dict(ssq_freqs=(0.0, 1 / 12, 5)), dict(ssq_freqs=(0.1, 1 / 12)), dict(gamma=-1.0),
               dict(gamma=np.nan), dict(ssq_freqs=(0.01, 1e-4, 32768))):
        with pytest.raises(ValueError):
            pycwt_amd.ssq_cwt_torch(x, 1.0, **kw)
        if "ssq_freqs" not in kw or kw["ssq_freqs"][-1] != 32768:
            with pytest.raises(ValueError):                                           # what ssq_cwt raises
                pycwt_amd.ssq_cwt(x.cpu().numpy(), 1.0, **kw)
    for kw in (dict(pad=False), dict(hop=2), dict(pool=2), dict(scales=x), dict(f0=x)):
        with pytest.raises(TypeError):
            pycwt_amd.ssq_cwt_torch(x, 1.0, **kw)
    with pytest.raises(TypeError):
        pycwt_amd.ssq_cwt_torch(x.cpu().numpy(), 1.0)
    with pytest.raises(ValueError):
        pycwt_amd.issq_cwt_torch(torch.zeros((4, 8), dtype=torch.complex128), 1.0, band=(0.1, 0.2))   # a band without the frequencies


def check_nonfinite_signal(torch, device):
    """a non-finite sample: NaN in all of that signal's Tx and gradient; the other signal of the batch as alone"""
    import pycwt_amd
    xs = np.stack([signal(128, 4, 64), signal(128, 5, 64)])
    xs[0, 17] = np.inf
    xt = torch.tensor(xs, device=device, requires_grad=True)
    Tx = pycwt_amd.ssq_cwt_torch(xt, 1.0)[0]
    Tx.abs().sum().backward()
    x1 = torch.tensor(xs[1], device=device, requires_grad=True)
    T1 = pycwt_amd.ssq_cwt_torch(x1, 1.0)[0]
    T1.abs().sum().backward()
    assert torch.isnan(Tx[0].real).all() and torch.isnan(Tx[0].imag).all() and torch.isnan(xt.grad[0]).all()
    assert torch.equal(Tx[1], T1) and torch.equal(xt.grad[1], x1.grad)


def check_torch_backward_exact(torch, device, n0, name, prec, batch, dj=1 / 4, seed=41):
    """x.grad of Re sum conj(C) Tx is, bit for bit, cwt_torch's backward on G_host[j, n] = w_j C[bins[j, n], n] built in NumPy from
    the saved map; a second call on the same engine gives the same bits; a loss written on Tx.conj() gives the same gradient"""
    import pycwt_amd
    from pycwt_amd import autograd
    real, cplx, eps = sc.types(prec)
    dt = 0.5
    rng = np.random.default_rng(seed)
    xs = np.stack([signal(n0, seed + b, prec) for b in range(batch or 1)])
    xs = xs if batch else xs[0]

    def grad(conj=False):
        xt = torch.tensor(xs, device=device, requires_grad=True)
        Tx = pycwt_amd.ssq_cwt_torch(xt, dt, dj, wavelet=name)[0]
        if grad.C is None:
            grad.C = torch.tensor((rng.standard_normal(tuple(Tx.shape)) + 1j * rng.standard_normal(tuple(Tx.shape))).astype(cplx), device=device)
        loss = (grad.C * Tx.conj()).real.sum() if conj else (grad.C.conj() * Tx).real.sum()       # Re(C conj(T)) = Re(conj(C) T)
        bins = autograd._ssq_saved_bins(Tx).cpu().numpy()
        loss.backward()
        return xt.grad.cpu().numpy(), bins, tuple(Tx.shape)
    grad.C = None
    g1, bins, shape = grad()
    g2, bins2, _ = grad()
    g3 = grad(conj=True)[0]
    assert same_bits(g1, g2) and np.array_equal(bins, bins2)
    assert same_bits(g1, g3)
    assert np.isfinite(g1).all() and np.abs(g1).max() > 0
    Cn = grad.C.cpu().numpy()
    for b in range(batch or 1):
        xb, Cb, bb, gb = (a[b] if batch else a for a in (xs, Cn, bins, g1))
        x2 = torch.tensor(xb, device=device, requires_grad=True)
        W2, sj = pycwt_amd.cwt_torch(x2, dt, dj, wavelet=name)[:2]
        G_host = gather_reference(Cb, bb, 1.0 / np.sqrt(sj), real)[0]
        W2.backward(torch.tensor(G_host, device=device))
        assert same_bits(gb, x2.grad.cpu().numpy()), b


def check_torch_large(torch, device, n0=1 << 18, rows=64, sample=4096, seed=51):
    """2^18 samples x 64 scales: the saved map and Tx on a seeded sample of columns against the host definition on the engine's own
    W and dW; x.grad bit for bit through cwt_torch's backward on the cotangent gathered on the device with torch's own indexing"""
    import pycwt_amd
    from pycwt_amd import autograd, wavelet
    real, cplx, eps = sc.types(64)
    dt, dj = 1.0, 1 / 4
    x = signal(n0, seed, 64)
    kw = dict(dj=dj, J=rows - 1, wavelet="morlet")
    xt = torch.tensor(x, device=device, requires_grad=True)
    keep = wavelet.SSQ_CHUNK_ROWS
    try:
        wavelet.SSQ_CHUNK_ROWS = 1 << 20                       # one chunk: dW with the bits of one transform_rows call
        Tx, fs, sj, freqs, coi = pycwt_amd.ssq_cwt_torch(xt, dt, **kw)
    finally:
        wavelet.SSQ_CHUNK_ROWS = keep
    bins = autograd._ssq_saved_bins(Tx)
    nf = fs.size
    assert sj.size == rows and bins.shape == (rows, n0) and Tx.shape == (nf, n0)
    cols = torch.tensor(np.sort(np.random.default_rng(seed).choice(n0, size=sample, replace=False)), device=device)
    W, sj2 = pycwt_amd.cwt_torch(xt.detach(), dt, **kw)[:2]
    eng = engine_of(xt, n0)
    xhat = torch.empty(eng.plan.nfft, dtype=W.dtype, device=device)
    dW = torch.empty_like(W)
    eng.forward(xt.detach(), n0, xhat)
    eng.plan.spectrum_derivative(xhat.data_ptr(), dt, xhat.data_ptr())
    eng.plan.transform_rows(xhat.data_ptr(), sc.MOTHERS["morlet"][0], 6.0, dt, sj, dW.data_ptr(), n0, n0)
    ref = sc.Reference(W[:, cols].cpu().numpy(), dW[:, cols].cpu().numpy(), 1.0 / np.sqrt(sj), host_gamma(x, 64), float(fs[0]), dj, nf)
    assert np.array_equal(bins[:, cols].cpu().numpy(), expected_bins(ref))
    T = Tx.detach()[:, cols].cpu().numpy()
    sc.assert_cells(T, ref, eps)
    assert np.all(T[ref.m == 0] == 0)
    del dW, xhat
    # the exact route of the backward: G[j, n] = w_j C[bins[j, n], n], w in the plan's precision, one product per component
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = torch.complex(torch.randn((nf, n0), generator=g, dtype=torch.float64), torch.randn((nf, n0), generator=g, dtype=torch.float64)).to(device)
    (C.conj() * Tx).real.sum().backward()
    k = bins.to(torch.int64)
    picked = torch.gather(C, 0, k.clamp(min=0))
    wt = torch.tensor(1.0 / np.sqrt(sj), device=device)[:, None]
    G = torch.where(k >= 0, torch.complex(wt * picked.real, wt * picked.imag), torch.zeros((), dtype=C.dtype, device=device))
    x2 = torch.tensor(x, device=device, requires_grad=True)
    pycwt_amd.cwt_torch(x2, dt, **kw)[0].backward(G)
    assert torch.equal(xt.grad, x2.grad) and bool(torch.isfinite(xt.grad).all()) and float(xt.grad.abs().max()) > 0


def check_torch_stream(torch, device):
    """forward and backward on a stream that is not the default one, back to back without a host synchronisation in between: the
    bits of the same on the default stream"""
    import pycwt_amd
    x = signal(3000, 61, 64)
    gamma = host_gamma(x, 64)                                   # (an explicit gamma: the default reads the signal's std back)
    rng = np.random.default_rng(62)

    def run():
        xt = torch.tensor(x, device=device, requires_grad=True)
        Tx = pycwt_amd.ssq_cwt_torch(xt, 1.0, 1 / 4, gamma=gamma)[0]
        if run.C is None:
            run.C = torch.tensor(rng.standard_normal(tuple(Tx.shape)) + 1j * rng.standard_normal(tuple(Tx.shape)), device=device)
        (run.C.conj() * Tx).real.sum().backward()
        return Tx.detach(), xt.grad
    run.C = None
    T0, g0 = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        T1, g1 = run()
        T2, g2 = run()
    side.synchronize()
    assert torch.equal(T0, T1) and torch.equal(g0, g1) and torch.equal(T0, T2) and torch.equal(g0, g2)
    run()                                                       # and back on the default stream
    torch.cuda.synchronize()


def tones(n0=4096):
    """(x, dx): two tones plus a slow chirp; the direction is a third tone"""
    t = np.arange(n0)
    x = np.cos(2 * np.pi * 0.031 * t + 0.3) + 0.7 * np.cos(2 * np.pi * 0.117 * t + 1.1) + 0.5 * np.cos(2 * np.pi * (0.05 * t + 0.5 * (0.02 / n0) * t * t))
    return x, np.cos(2 * np.pi * 0.071 * t + 0.5)


INDEPENDENT_CONSTANT = 0.0165   # measured on the emulator, the largest of 16 cotangents (profiles/ssq_grad_accuracy.txt), in units
INDEPENDENT_MARGIN = 8          # of eps sum |C| |T| / h; the GPU's summation order inside the adjoint differs from the emulator's
INDEPENDENT_SEEDS = (0, 1, 2, 3)


def torch_independent_route(torch, device, seeds=(3,)):
    """[(error, eps sum |C| |T| / h, <x.grad, dx>)] per seed of C for the finite difference Re sum conj(C) (Tx(x + h dx) - Tx(x)) / h
    against <x.grad, dx> at a point where the map of x + h dx equals the map of x (asserted): T is exactly linear between the two,
    the error is rounding"""
    import pycwt_amd
    from pycwt_amd import autograd
    x, dx = tones()
    h = 1e-8 * np.linalg.norm(x) / np.linalg.norm(dx)
    gamma = 1e-3 * float(np.std(x))                                    # well above the rounding floor sqrt(eps) std(x)
    kw = dict(dj=1 / 4, wavelet="morlet", gamma=gamma)
    xt = torch.tensor(x, device=device, requires_grad=True)
    Tx = pycwt_amd.ssq_cwt_torch(xt, 1.0, **kw)[0]
    x2 = torch.tensor(x + h * dx, device=device, requires_grad=True)
    Tx2 = pycwt_amd.ssq_cwt_torch(x2, 1.0, **kw)[0]
    assert torch.equal(autograd._ssq_saved_bins(Tx), autograd._ssq_saved_bins(Tx2))              # the precondition
    assert (autograd._ssq_saved_bins(Tx) >= 0).float().mean() > 0.5
    T1, T2 = Tx.detach().cpu().numpy(), Tx2.detach().cpu().numpy()
    d = T2 - T1
    out = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        C = rng.standard_normal(tuple(Tx.shape)) + 1j * rng.standard_normal(tuple(Tx.shape))
        xt.grad = None
        (torch.tensor(C, device=device).conj() * Tx).real.sum().backward(retain_graph=True)
        fd = (C.real.astype(L) * d.real.astype(L) + C.imag.astype(L) * d.imag.astype(L)).sum() / L(h)
        an = (xt.grad.cpu().numpy().astype(L) * dx.astype(L)).sum()
        unit = L(np.finfo(np.float64).eps) * (np.abs(C).astype(L) * np.abs(T1).astype(L)).sum() / L(h)
        out.append((float(abs(fd - an)), float(unit), float(an)))
    return out


def check_issq_torch(torch, device):
    """issq_cwt_torch against issq_cwt on the host, with and without a band: 8 nf eps max_n sum_k |Tx[k, n]|; gradcheck alone"""
    import pycwt_amd
    rng = np.random.default_rng(12)
    nf, n0 = 9, 200
    fs = 0.05 * 2.0 ** ((1 / 6) * np.arange(nf))
    Tn = rng.standard_normal((nf, n0)) + 1j * rng.standard_normal((nf, n0))
    tol = 8 * nf * np.finfo(np.float64).eps * np.abs(Tn).sum(axis=0).max()
    for name in TORCH_MOTHERS:
        for kw in (dict(), dict(ssq_freqs=fs, band=(0.06, 0.2))):
            got = pycwt_amd.issq_cwt_torch(torch.tensor(Tn, device=device), 0.5, 1 / 6, name, **kw)
            want = pycwt_amd.issq_cwt(Tn, 0.5, 1 / 6, name, **kw)
            assert got.shape == (n0,) and np.abs(got.cpu().numpy() - want).max() <= tol
    both = pycwt_amd.issq_cwt_torch(torch.tensor(np.stack([Tn, 2 * Tn]), device=device), 0.5, 1 / 6)
    assert both.shape == (2, n0) and torch.equal(both[1], 2 * both[0])
    T = torch.tensor(rng.standard_normal((5, 40)) + 1j * rng.standard_normal((5, 40)), device=device, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.issq_cwt_torch(t, 0.5, 1 / 6), (T,))
    assert torch.autograd.gradcheck(lambda t: pycwt_amd.issq_cwt_torch(t, 0.5, 1 / 6, ssq_freqs=fs[:5], band=(0.06, 0.2)), (T,))
