"""Shared by tests/test_shrink_grad_emulated.py, tests/test_shrink_grad_schedules_emulated.py, tests/test_shrink_grad_gpu.py and
tests/perf/shrink_grad_accuracy.py: the cases, references and bounds of the gradient of wavelet shrinkage --
cwt_icwt_shrink_adjoint (include/cwt_hip.h) and the torch entry points icwt_torch / icwt_shrink_torch / denoise_torch.

REFERENCE.  The closed form of include/cwt_hip.h in NumPy long double on the inputs rounded to the plan's precision T (W, lambda,
gy, T(coeff), T(1 / sqrt(s_j))).  `inputs` builds W so that the reference and the kernel take the same decision for every entry:
lambda_j = 5 2^k, so l2 = 25 4^k is exact; every entry has |v / l2 - 1| >= 2^-10 (those that fell closer are moved away), except
the planted ones W = (+-3 +- 4i) 2^k and (+-4 +- 3i) 2^k, for which v == l2 holds exactly in both precisions and every mode drops
them (v > l2 is false; lambda / sqrt(v) = 1 and l2 / v = 1 exactly, f = 0).  No entry is excluded from a comparison.

BOUNDS, counted in units of u = eps / 2 (one rounding) for the operation order of cwt_kernels_shrink_grad.hpp; fused
multiply-adds only remove roundings.  t = (T(coeff) w_j) gy[n] carries 2.  v = fma(a, a, b b): 2.
  hard, plain   G.re = t: 2                                                                                       -> 3 u |t|
  soft          r = sqrt(v): 2 / 2 + 1 = 2; q = lambda / r: 3; f = 1 - q: 3 q + 1 <= 4 (absolute; q, f <= 1); ir = 1 / r: 3;
                u = a ir, s = b ir: 4; q u: 8; (q u) u: 13 (<= q <= 1); gr = f + (q u) u: 4 + 13 + 1 = 18 (gr <= 1);
                t gr: 18 + (2 + 1) gr <= 21; gi = (q u) s: 13, t gi: <= 15                                        -> 22 u |t|
                gl = -u: 4; t gl: 4 + 2 + 1 = 7                                                                   -> 8 u |term|
  garrote       l2: 1; q = l2 / v: 4; f: 4 q + 1 <= 5; p = a / v: 3; a p: 4 (<= 1); 2 q (a p): 9 relative of <= 2: 18;
                gr = f + 2 q (a p): 5 + 18 + 2 = 25 (gr <= 2); t gr: 25 + 3 x 2 = 31; gi: 9 + 3 = 12             -> 32 u |t|
                gl = -(2 lambda) p: 4; t gl: 7                                                                    -> 8 u |term|
(the last step of each line rounds the first-order count up by one for the second-order terms).  glambda[j] adds its terms in a
tree of depth 7 (a thread's 8 columns) + 8 (256 threads) = 15 roundings in T, then the slices in double:
  |glambda - sum term| <= (8 + 15 + (slices - 1) eps_double / eps_T) u sum |term|.
No margin is taken over these counts; the measured worst cases (tests/perf/shrink_grad_accuracy.py ->
profiles/shrink_grad_accuracy.txt) are a record, the tests assert the counts.
"""
import ctypes as C
import os
import re

import numpy as np

import shrink_common as sc
from conftest import ROOT
from shrink_common import Dev, EINVAL, L, MODES, PAD, PRECS, SENTINEL, launch_log, padded, types  # noqa: F401

ROWS = (1, 7, 8, 9)
NCOLS = (1, 255, 256, 257, 2047, 2048, 2049, 4099)                 # around the 256-thread workgroup and the 2048-column slice
PATTERNS = ("mixed", "zero", "inf")
CASES = [(r, n, p) for r in ROWS for n in NCOLS for p in PATTERNS]
LARGE = (3, (1 << 17) + 3)                                         # GPU only: one row spans 65 slices
COEFF = 0.37
SLICE = 2048
SJ = 2.0 * 2.0 ** (np.arange(16) / 4.0)
G_BOUND = {None: 3, "hard": 3, "soft": 22, "garrote": 32}          # in u = eps / 2, relative to |t|
TERM_BOUND = {"hard": 0, "soft": 8, "garrote": 8}                  # per term of glambda, relative to |term|
SUM_DEPTH = 15
ACCURACY_FILE = os.path.join(ROOT, "profiles", "shrink_grad_accuracy.txt")
HEADER = os.path.join(ROOT, "pycwt_amd", "csrc", "cwt_kernels_shrink_grad.hpp")
KERNELS = {"shgrad_rows", "shgrad_sum"}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(nrows, ncols, prec, pattern, seed=17):
    """(W, sj, lam, gy, planted): module docstring.  "mixed": every fifth row lambda = 0, every seventh +inf, as
    shrink_common.thresholds; planted: the boolean mask of the entries put exactly on their threshold"""
    real, cplx, eps = types(prec)
    rng = np.random.default_rng([seed, nrows, ncols, prec])
    W = (rng.standard_normal((nrows, ncols)) + 1j * rng.standard_normal((nrows, ncols))).astype(cplx)
    gy = rng.standard_normal(ncols).astype(real)
    sj = SJ[:nrows].copy()
    planted = np.zeros((nrows, ncols), dtype=bool)
    if pattern == "zero":
        return W, sj, np.zeros(nrows, dtype=real), gy, planted
    if pattern == "inf":
        return W, sj, np.full(nrows, np.inf, dtype=real), gy, planted
    lam = np.empty(nrows, dtype=real)
    shapes = [(3, 4), (-3, 4), (4, -3), (-4, -3), (3, -4), (-4, 3)]
    for j in range(nrows):
        k = int(np.round(np.log2(np.median(np.abs(W[j])) / 5.0)))
        lam[j] = real(5.0 * 2.0 ** k)
        l2 = L(25.0) * L(4.0) ** k
        near = np.abs(sc.abs2_long(W[j:j + 1])[0] / l2 - 1) < L(2.0) ** -9
        W[j, near] = (W[j, near] * cplx(1.25)).astype(cplx)
        cols = rng.choice(ncols, size=min(6, ncols // 2), replace=False)
        for i, c in enumerate(cols):
            W[j, c] = cplx(complex(*shapes[i % len(shapes)]) * 2.0 ** k)
            planted[j, c] = True
    lam[3::5] = 0
    lam[5::7] = np.inf
    planted[~np.isfinite(lam) | (lam == 0)] = False
    # the construction: on the threshold exactly, or well away from it
    v = sc.abs2_long(W)
    l2 = lam.astype(L)[:, None] ** 2
    fin = np.isfinite(lam) & (lam > 0)
    assert np.all(v[planted] == np.broadcast_to(l2, v.shape)[planted])
    with np.errstate(all="ignore"):
        away = np.abs(v / l2 - 1) >= L(2.0) ** -10
    assert np.all(away[fin] | planted[fin]) and 2.0 ** -10 > 128 * eps
    return W, sj, lam, gy, planted


def weights(sj, coeff, real):
    """(T(coeff), T(1 / sqrt(s_j))) as the library rounds them"""
    return real(coeff), (1.0 / np.sqrt(np.asarray(sj, dtype=np.float64))).astype(real)


def reference(W, sj, lam, mode, coeff, gy):
    """(G.re, G.im, terms of glambda, |t|) in long double; mode None: the plain inverse"""
    real = W.real.dtype.type
    a, b = W.real.astype(L), W.imag.astype(L)
    cT, wT = weights(sj, coeff, real)
    t = L(cT) * wT.astype(L)[:, None] * gy.astype(L)[None, :]
    one, zero = np.ones(W.shape, dtype=L), np.zeros(W.shape, dtype=L)
    if mode is None:
        return t * one, zero, zero, np.abs(t)
    v = a * a + b * b
    lm = np.broadcast_to(lam.astype(L)[:, None], W.shape)
    with np.errstate(all="ignore"):
        l2 = lm * lm
        kept = (v > l2) & (v > 0)
        r = np.sqrt(v)
        if mode == "hard":
            fr, fi, fl = one, zero, zero
        elif mode == "soft":
            fr, fi, fl = (1 - lm / r) + lm * a * a / r ** 3, lm * a * b / r ** 3, -a / r
        else:
            fr, fi, fl = (1 - l2 / v) + 2 * l2 * a * a / (v * v), 2 * l2 * a * b / (v * v), -2 * lm * a / v
        fr, fi, fl = (np.where(kept, f, zero) for f in (fr, fi, fl))
        return t * fr, t * fi, t * fl, np.abs(t)


# ---- the export --------------------------------------------------------------------------------------------------------------------
def run_adjoint(dev, W, sj, lam, mode, gy, coeff=COEFF, want_glambda=True, inplace=False, start=None, chunks=None):
    """cwt_icwt_shrink_adjoint with ldw = ldg = ncols + PAD (the padding of W NaN), rows in `chunks` (None: one call).  G has a
    guard row of sentinels before and after it and sentinels in its padding, glambda a guard element on either side; all
    asserted intact.  inplace: G_dev = W_dev (the NaN padding must survive).  start: glambda before the call, accumulate = 1.
    lam None: lambda_dev = NULL.  Returns (G, glambda or None)."""
    nrows, ncols = W.shape
    ld = ncols + PAD
    cs = np.dtype(dev.cplx).itemsize
    nan = complex(np.nan, np.nan)
    Wp = padded(W, PAD, nan)
    Wd = dev.up(Wp)
    gd = dev.up(gy.astype(dev.real))
    ld_dev = None if lam is None else dev.up(lam.astype(dev.real))
    Gd = Wd if inplace else dev.up(np.full((nrows + 2, ld), SENTINEL, dtype=dev.cplx))
    g0 = Gd.ptr if inplace else Gd.ptr + ld * cs
    gl0 = np.full(nrows + 2, SENTINEL, dtype=np.float64)
    if start is not None:
        gl0[1:-1] = start
    gld = dev.up(gl0) if want_glambda else None
    es = np.dtype(dev.real).itemsize
    a = 0
    for cnt in (chunks or [nrows]):
        dev.plan.icwt_shrink_adjoint(Wd.ptr + a * ld * cs, ld, ncols, sj[a:a + cnt], None if ld_dev is None else ld_dev.ptr + a * es,
                                     mode if mode is not None else 0, coeff, gd.ptr, g0 + a * ld * cs, ld,
                                     None if gld is None else gld.ptr + (1 + a) * 8, start is not None)
        a += cnt
    assert a == nrows
    if inplace:
        out = Gd.download(dev.plan, (nrows, ld), dev.cplx)
        assert np.isnan(out[:, ncols:].real).all() and np.isnan(out[:, ncols:].imag).all()
        G = out[:, :ncols]
    else:
        out = Gd.download(dev.plan, (nrows + 2, ld), dev.cplx)
        assert np.all(out[0] == SENTINEL) and np.all(out[-1] == SENTINEL) and np.all(out[:, ncols:] == SENTINEL)
        G = out[1:-1, :ncols]
        assert same_bits(Wd.download(dev.plan, Wp.shape, dev.cplx), Wp)                                   # inputs are inputs
    gl = None
    if want_glambda:
        full = gld.download(dev.plan, (nrows + 2,), np.float64)
        assert full[0] == SENTINEL and full[-1] == SENTINEL
        gl = full[1:-1]
    dev.release()
    return np.ascontiguousarray(G), gl


def glambda_bound_units(mode, ncols, eps):
    slices = -(-ncols // SLICE)
    return TERM_BOUND[mode] + SUM_DEPTH + (slices - 1) * float(np.finfo(np.float64).eps) / eps


def compare(G, gl, W, sj, lam, mode, coeff, gy, eps, where=None):
    """(worst error of G, of glambda) in units of u relative to |t| and to sum |term|; asserts the bounds.  where: the entries
    that take part (None: all -- no entry is excluded)"""
    gre, gim, terms, tabs = reference(W, sj, lam, mode, coeff, gy)
    u = L(eps) / 2
    take = np.ones(W.shape, dtype=bool) if where is None else where
    if where is None:
        assert take.all() and np.all(tabs > 0) and np.isfinite(G.real).all() and np.isfinite(G.imag).all()
    err = np.maximum(np.abs(G.real.astype(L) - gre), np.abs(G.imag.astype(L) - gim))
    worst_g = float((err[take] / tabs[take]).max() / u)
    assert worst_g <= G_BOUND[mode], (mode, worst_g, G_BOUND[mode])
    worst_l = 0.0
    if gl is not None and where is None:
        total, mag = terms.sum(axis=1), np.abs(terms).sum(axis=1)
        d = np.abs(gl.astype(L) - total)
        assert np.all(d[mag == 0] == 0)
        if (mag > 0).any():
            worst_l = float((d[mag > 0] / mag[mag > 0]).max() / u)
        bound = glambda_bound_units(mode, W.shape[1], eps)
        assert worst_l <= bound, (mode, worst_l, bound)
    return worst_g, worst_l


def check_closed_form(dev, nrows, ncols, pattern, mode):
    """the export against the closed form, every entry; returns the worst errors in u"""
    W, sj, lam, gy, planted = inputs(nrows, ncols, dev.prec, pattern)
    G, gl = run_adjoint(dev, W, sj, lam, mode, gy)
    assert np.all(G[planted] == 0)                                  # on the threshold: dropped, as the forward drops it
    if pattern == "inf":
        assert np.all(G == 0) and np.all(gl == 0)
    if mode == "hard":
        assert np.all(gl == 0) and np.all(G.imag == 0) and not np.signbit(G.imag).any()
    out = compare(G, gl, W, sj, lam, mode, COEFF, gy, dev.eps)
    print(f"fp{dev.prec} {nrows} x {ncols} {pattern} {mode}: G {out[0]:.2f} u (bound {G_BOUND[mode]}), glambda {out[1]:.2f} u "
          f"(bound {glambda_bound_units(mode, ncols, dev.eps):.2f})")
    return out


def check_forward_agrees_on_planted(dev, mode):
    """the forward drops the planted entries too: y of W equals y of W with the planted entries zeroed, bit for bit"""
    W, sj, lam, gy, planted = inputs(9, 4099, dev.prec, "mixed")
    W0 = W.copy()
    W0[planted] = 0
    assert planted.sum() >= 30
    assert same_bits(sc.run_shrink(dev, W, sj, lam, mode), sc.run_shrink(dev, W0, sj, lam, mode))


def check_transpose(dev, nrows, ncols):
    """the exact linear case.  Mode 0 with every lambda = 0, and lambda_dev = NULL: G.im is +0 and G.re = (T(coeff) w_j) gy[n] bit
    for bit in NumPy's arithmetic of T; sum_n y[n] gy[n] = Re sum conj(G) W within the counted rounding: y[n] carries one
    product, at most ceil(rows / 8) + 3 additions and the factor per term (7 u for rows <= 16), G.re 2 u, so 9 -> 10 u
    sum |coeff w_j gy[n] Re W[j, n]|"""
    W, sj, _, gy, _ = inputs(nrows, ncols, dev.prec, "zero")
    zero = np.zeros(nrows, dtype=dev.real)
    cT, wT = weights(sj, COEFF, dev.real)
    want = (cT * wT)[:, None] * gy[None, :]
    assert want.dtype == dev.real
    y, red = sc.run_shrink(dev, W, sj, zero, "hard", reduce_too=True)
    assert same_bits(y, red)
    for lam, mode in ((zero, "hard"), (None, None)):
        G, _ = run_adjoint(dev, W, sj, lam, mode, gy, want_glambda=lam is not None)
        assert same_bits(np.ascontiguousarray(G.real), want), mode
        assert np.all(G.imag == 0) and not np.signbit(G.imag).any(), mode
        lhs = (y.astype(L) * gy.astype(L)).sum()
        rhs = (G.real.astype(L) * W.real.astype(L)).sum()
        bound = 10 * L(dev.eps) / 2 * (np.abs(want).astype(L) * np.abs(W.real).astype(L)).sum()
        assert abs(lhs - rhs) <= bound, (float(lhs), float(rhs), float(bound))


def check_inplace(dev, mode):
    W, sj, lam, gy, _ = inputs(9, 4099, dev.prec, "mixed")
    G, gl = run_adjoint(dev, W, sj, lam, mode, gy)
    G2, gl2 = run_adjoint(dev, W, sj, lam, mode, gy, inplace=True)
    assert same_bits(G, G2) and same_bits(gl, gl2)


def check_independence(dev, mode):
    """a row's bits do not depend on the rows around it or on how the rows are split over calls; accumulate = 1 adds in double"""
    W, sj, lam, gy, _ = inputs(9, 4099, dev.prec, "mixed")
    G, gl = run_adjoint(dev, W, sj, lam, mode, gy)
    for chunks in ([1] * 9, [1, 4, 4]):
        G2, gl2 = run_adjoint(dev, W, sj, lam, mode, gy, chunks=chunks)
        assert same_bits(G, G2) and same_bits(gl, gl2), chunks
    for j in (0, 4, 8):
        Gj, glj = run_adjoint(dev, W[j:j + 1], sj[j:j + 1], lam[j:j + 1], mode, gy)
        assert same_bits(Gj[0], G[j]) and glj[0] == gl[j], j
    W2 = inputs(9, 4099, dev.prec, "mixed", seed=18)[0]
    lam2 = lam.copy()
    _, second = run_adjoint(dev, W2, sj, lam2, mode, gy)
    _, both = run_adjoint(dev, W2, sj, lam2, mode, gy, start=gl)
    assert same_bits(both, gl + second)
    Gn, none = run_adjoint(dev, W, sj, lam, mode, gy, want_glambda=False)
    assert none is None and same_bits(Gn, G)


def check_special_entries(dev):
    """v = 0, signed zeros, a NaN entry, a NaN lambda, lambda = +inf, a NaN and a zero in gy"""
    rng = np.random.default_rng(9)
    W = (rng.standard_normal((4, 8)) + 1j * rng.standard_normal((4, 8))).astype(dev.cplx)
    W[1, 2] = 0
    W[0, 1] = complex(-0.0, 1.5)
    W[0, 3] = complex(2.0, -0.0)
    W[1, 7] = complex(-0.0, -0.0)
    W[2, 4] = complex(1.0, np.nan)
    sj = np.array([1.0, 2.0, 4.0, 8.0])
    gy = rng.standard_normal(8).astype(dev.real)
    gy[6] = 0
    lam = np.array([0.3, 0.5, 0.2, np.inf], dtype=dev.real)
    ok = np.ones((4, 8), dtype=bool)
    ok[2, 4] = False
    for mode in MODES:
        G, gl = run_adjoint(dev, W, sj, lam, mode, gy, coeff=1.0)
        assert np.isnan(G[2, 4].real) and np.isnan(G[2, 4].imag) and np.isnan(gl[2])
        assert np.isfinite(G[ok].real).all() and np.isfinite(G[ok].imag).all() and np.isfinite(gl[[0, 1, 3]]).all()
        assert np.all(G[3] == 0) and gl[3] == 0                      # lambda = +inf
        assert G[1, 2] == 0 and G[1, 7] == 0                         # v = 0
        assert np.all(G[:, 6][ok[:, 6]] == 0)                        # gy = 0
        Wf = np.where(ok, W, 1)
        take = ok & (gy != 0)[None, :]
        compare(G, None, Wf, sj, lam, mode, 1.0, gy, dev.eps, where=take)
        gre, gim, terms, _ = reference(Wf, sj, lam, mode, 1.0, gy)
        for j in (0, 1):
            mag = np.abs(terms[j]).sum()
            assert abs(L(gl[j]) - terms[j].sum()) <= glambda_bound_units(mode, 8, dev.eps) * L(dev.eps) / 2 * mag
        lam_nan = lam.copy()
        lam_nan[1] = np.nan
        G2, gl2 = run_adjoint(dev, W, sj, lam_nan, mode, gy, coeff=1.0)
        assert np.isnan(G2[1].real).all() and np.isnan(G2[1].imag).all() and np.isnan(gl2[1])
        rest = [0, 2, 3]
        assert same_bits(G2[rest], G[rest]) and same_bits(gl2[rest], gl[rest])
        gy_nan = gy.copy()
        gy_nan[5] = np.nan
        G3, gl3 = run_adjoint(dev, W, sj, lam, mode, gy_nan, coeff=1.0)
        assert np.isnan(G3[:, 5].real).all() and np.isnan(gl3).all()
        cols = [c for c in range(8) if c != 5]
        assert same_bits(np.ascontiguousarray(G3[:, cols]), np.ascontiguousarray(G[:, cols]))


def refusals(dev, nrows=3, ncols=257):
    """(label, return code) of every argument set the entry point refuses, and whether every buffer kept its bits"""
    W, sj, lam, gy, _ = inputs(nrows, ncols, dev.prec, "zero")
    ld = ncols + PAD
    Wp = padded(W, PAD, 0)
    gstart = np.full((nrows + 1, ld), SENTINEL, dtype=dev.cplx)
    lstart = np.full(nrows + 1, SENTINEL, dtype=np.float64)
    Wd, Gd, gld, lamd, gyd = dev.up(Wp), dev.up(gstart), dev.up(lstart), dev.up(lam), dev.up(gy)
    lib, h, P = dev.lib, dev.plan.h, C.c_void_p
    sp = sj.ctypes.data_as(C.POINTER(C.c_double))
    bad_scales = np.array([1.0, 0.0, 3.0][:nrows])
    nan_scales = np.array([1.0, np.nan, 3.0][:nrows])

    def call(W=Wd.ptr, ldw=ld, ncols=ncols, nrows=nrows, s=sp, lam=lamd.ptr, mode=1, gy=gyd.ptr, G=Gd.ptr, ldg=ld, gl=gld.ptr, plan=h):
        return lib.cwt_icwt_shrink_adjoint(plan, P(W), ldw, ncols, nrows, s, P(lam), mode, 1.0, P(gy), P(G), ldg, P(gl), 0)

    out = [("mode 3", call(mode=3)), ("mode -1", call(mode=-1)), ("ncols 0", call(ncols=0)), ("nrows 0", call(nrows=0)),
           ("nrows > max_rows", call(nrows=dev.plan.max_rows + 1)), ("ldw < ncols", call(ldw=ncols - 1)),
           ("ldg < ncols", call(ldg=ncols - 1)), ("scale 0", call(s=bad_scales.ctypes.data_as(C.POINTER(C.c_double)))),
           ("scale nan", call(s=nan_scales.ctypes.data_as(C.POINTER(C.c_double)))), ("W NULL", call(W=None)),
           ("W NULL without lambda", call(W=None, lam=None, gl=None)), ("gy NULL", call(gy=None)), ("G NULL", call(G=None)),
           ("scales NULL", call(s=None)), ("plan NULL", call(plan=None)), ("glambda without lambda", call(lam=None)),
           ("mode 3 without lambda", call(lam=None, gl=None, mode=3))]
    dev.plan.sync()
    untouched = (same_bits(Gd.download(dev.plan, gstart.shape, dev.cplx), gstart) and same_bits(gld.download(dev.plan, lstart.shape, np.float64), lstart)
                 and same_bits(Wd.download(dev.plan, Wp.shape, dev.cplx), Wp))
    assert call() == 0 and call(lam=None, gl=None) == 0 and call(gl=None) == 0           # the argument sets around them are accepted
    dev.plan.sync()
    dev.release()
    return out, untouched


# ---- a live plan -------------------------------------------------------------------------------------------------------------------
def _adjoint_then_rows(dev, x, rows, mode):
    """transform -> cwt_icwt_shrink_adjoint in place with glambda -> cwt_adjoint_rows, buffers on the device throughout"""
    from oracle import cwt_oracle as orc
    sj = sc.SJ[:rows]
    n0 = sc.N0
    es, cs = np.dtype(dev.real).itemsize, np.dtype(dev.cplx).itemsize
    rng = np.random.default_rng(rows)
    gy = rng.standard_normal(n0).astype(dev.real)
    lam = np.full(rows, 0.8, dtype=dev.real)
    xd, Wd = dev.up(x.astype(dev.real)), dev.up(np.zeros((rows, n0), dtype=dev.cplx))
    gd, lamd, gld, xb = dev.up(gy), dev.up(lam), dev.up(np.zeros(rows)), dev.up(np.zeros(n0, dtype=dev.real))
    dev.plan.transform(xd.ptr, n0, orc.MORLET, 6.0, 1.0, sj, None, Wd.ptr, n0, n0)
    dev.plan.icwt_shrink_adjoint(Wd.ptr, n0, n0, sj, lamd.ptr, mode, 1.0, gd.ptr, Wd.ptr, n0, gld.ptr)
    dev.plan.adjoint_rows(Wd.ptr, 1, rows * n0, n0, n0, orc.MORLET, 6.0, 1.0, sj, xb.ptr, n0)
    out = (Wd.download(dev.plan, (rows, n0), dev.cplx), gld.download(dev.plan, (rows,), np.float64), xb.download(dev.plan, (n0,), dev.real))
    dev.release()
    assert np.isfinite(out[2]).all() and np.abs(out[2]).max() > 0
    return out


def check_live_plan_sequence(lib, prec):
    """the new call between cwt_icwt_shrink, cwt_row_order_statistics and cwt_adjoint_rows on one plan, its scratch sized small
    (3 x 257: one slice a row) and then large (40 rows x 4099: three slices a row) and small again: bit for bit what fresh plans give"""
    x = sc.noise_signal(8)
    Ws, sjs, lams, gys, _ = inputs(3, 257, prec, "mixed")
    Wl, sjl, laml, gyl, _ = inputs(9, 4099, prec, "mixed")
    ranks = np.array([0, 2049, 4098])
    steps = [("small", lambda d: run_adjoint(d, Ws, sjs, lams, "soft", gys)),
             ("shrink", lambda d: (sc.run_shrink(d, Wl, sjl, laml, "soft"),)),
             ("select", lambda d: (sc.run_select(d, Wl, ranks, True),)),
             ("rows", lambda d: _adjoint_then_rows(d, x, 40, "garrote")),
             ("large", lambda d: run_adjoint(d, Wl, sjl, laml, "garrote", gyl)),
             ("small", lambda d: run_adjoint(d, Ws, sjs, lams, "soft", gys)),
             ("shrink", lambda d: (sc.run_shrink(d, Wl, sjl, laml, "soft"),)),
             ("rows", lambda d: _adjoint_then_rows(d, x, 40, "garrote"))]
    with Dev(lib, sc.NFFT, prec, max_rows=sc.ROWS_W) as dev:
        live = [(name, f(dev)) for name, f in steps]
    fresh = {}
    for name, f in steps:
        if name not in fresh:
            with Dev(lib, sc.NFFT, prec, max_rows=sc.ROWS_W) as dev:
                fresh[name] = f(dev)
    for name, got in live:
        for a, b in zip(got, fresh[name]):
            assert same_bits(a, b), name


# ---- schedules ---------------------------------------------------------------------------------------------------------------------
def schedule_case(lib, prec):
    """the three modes with glambda over 9 x 4099 entries (three slices a row: the LDS tree and shgrad_sum), the plain inverse, and
    3 x 257 without glambda: every kernel of cwt_kernels_shrink_grad.hpp, as bytes"""
    parts = []
    with Dev(lib, 16, prec, max_rows=16) as dev:
        W, sj, lam, gy, _ = inputs(9, 4099, prec, "mixed")
        for mode in MODES:
            parts += list(run_adjoint(dev, W, sj, lam, mode, gy))
        parts.append(run_adjoint(dev, W, sj, None, None, gy, want_glambda=False)[0])
        W, sj, lam, gy, _ = inputs(3, 257, prec, "mixed")
        parts.append(run_adjoint(dev, W, sj, lam, "soft", gy, want_glambda=False)[0])
    return np.concatenate([np.ascontiguousarray(p).view(np.uint8).ravel() for p in parts])


def kernels_of_the_header():
    text = open(HEADER).read()
    return set(re.findall(r"__global__[^{;]*?\b(shgrad_\w+)\s*\(", text)), re.findall(r"__global__[^{;]*?\b(k_\w+)\s*\(", text)


# ---- torch -------------------------------------------------------------------------------------------------------------------------
N0_T, DT_T, DJ_T, J_T = 300, 0.5, 1 / 4, 19                        # nfft 512, 20 rows
TORCH_MOTHERS = ("morlet", "paul", "dog")
TOL = sc.TOL


def mother_of(name):
    import pycwt_amd
    return {"morlet": pycwt_amd.Morlet(6), "paul": pycwt_amd.Paul(4), "dog": pycwt_amd.DOG(2)}[name]


def signals(batch, prec, seed=71):
    rng = np.random.default_rng(seed)
    t = np.arange(N0_T)
    xs = np.stack([np.sin(2 * np.pi * t / (16.0 + 8 * b)) + 0.4 * rng.standard_normal(N0_T) for b in range(batch or 1)])
    return (xs if batch else xs[0]).astype(types(prec)[0])


def kw(name):
    return dict(dj=DJ_T, J=J_T, wavelet=mother_of(name))


def check_torch_forward(torch, device, name, prec, batch):
    """denoise_torch = denoise and icwt_torch = icwt on the same data: thresholds bit for bit; the series bit for bit in fp64 and
    within one rounding of the factor and one of the product in fp32 (the shim multiplies in double there)"""
    import pycwt_amd
    real, cplx, eps = types(prec)
    xs = signals(batch, prec)
    xt = torch.tensor(xs, device=device)
    cases = [dict(mode="soft"), dict(mode="garrote", scale=0.7, noise_columns=(10, 210)), dict(mode="hard", noise_columns=(5, 300))]
    for case in cases:
        y, lam, sj, freqs, coi = pycwt_amd.denoise_torch(xt, DT_T, **kw(name), **case)
        assert y.shape == xt.shape and y.device == xt.device and y.real.dtype == xt.dtype and sj.size == J_T + 1
        assert lam.shape == xt.shape[:-1] + (sj.size,) and lam.dtype == torch.float64
        for b in range(batch or 1):
            xb, yb, lb = (a[b] if batch else a for a in (xs, y.cpu().numpy(), lam.cpu().numpy()))
            want = pycwt_amd.denoise(xb.astype(np.float64), DT_T, precision=prec, **kw(name), **case)
            assert np.array_equal(lb, want[1]), (name, case, b)
            for got, ref in zip((sj, freqs, coi), want[2:]):
                assert np.array_equal(got, ref)
            if prec == 64:
                assert np.array_equal(yb, want[0]), (name, case, b, float(np.abs(yb - want[0]).max()))
            else:
                assert np.all(np.abs(yb - want[0]) <= 1.01 * eps * np.abs(want[0])), (name, case, b)
    lam_rows = np.linspace(0.05, 0.6, J_T + 1)
    y, lam = pycwt_amd.denoise_torch(xt, DT_T, threshold=torch.tensor(lam_rows, device=device), mode="soft", **kw(name))[:2]
    W, sj = pycwt_amd.cwt_torch(xt, DT_T, **kw(name))[:2]
    rec = pycwt_amd.icwt_torch(W, sj, DT_T, DJ_T, mother_of(name))
    for b in range(batch or 1):
        xb, yb, rb, Wb = (a[b] if batch else a for a in (xs, y.cpu().numpy(), rec.cpu().numpy(), W.cpu().numpy()))
        want = pycwt_amd.denoise(xb.astype(np.float64), DT_T, precision=prec, threshold=lam_rows, mode="soft", **kw(name))[0]
        inv = pycwt_amd.icwt(Wb, sj, DT_T, DJ_T, mother_of(name), precision=prec)
        for got, ref in ((yb, want), (rb, inv)):
            if prec == 64:
                assert np.array_equal(got, ref), (name, b, float(np.abs(got - ref).max()))
            else:
                assert np.all(np.abs(got - ref) <= 1.01 * eps * np.abs(ref)), (name, b)
    assert tuple(lam.shape) == tuple(xt.shape[:-1]) + (J_T + 1,)


def check_torch_gradients(torch, device, name, prec, batch, mode):
    """gradients reach x, lam (rows,) and scale (), summed over the batch; per signal x.grad and lam.grad of denoise_torch are bit
    for bit those of cwt_torch -> icwt_shrink_torch, the path that keeps W"""
    import pycwt_amd
    real, cplx, eps = types(prec)
    xs = signals(batch, prec)
    nb = batch or 1
    rows = J_T + 1
    rng = np.random.default_rng(5)
    c = torch.tensor(rng.standard_normal(xs.shape).astype(real), device=device)
    lam0 = np.linspace(0.05, 0.5, nb * rows).reshape(nb, rows).astype(real)
    xt = torch.tensor(xs, device=device, requires_grad=True)
    lam_t = torch.tensor(lam0 if batch else lam0[0], device=device, requires_grad=True)
    y = pycwt_amd.denoise_torch(xt, DT_T, threshold=lam_t, mode=mode, **kw(name))[0]
    (y * c).sum().real.backward() if y.is_complex() else (y * c).sum().backward()
    assert xt.grad.shape == xt.shape and lam_t.grad.shape == lam_t.shape and lam_t.grad.dtype == lam_t.dtype
    assert bool(torch.isfinite(xt.grad).all()) and float(xt.grad.abs().max()) > 0
    if mode == "hard":
        assert bool((lam_t.grad == 0).all())
    else:
        assert float(lam_t.grad.abs().max()) > 0
    for b in range(nb):
        xb = torch.tensor(xs[b] if batch else xs, device=device, requires_grad=True)
        lb = torch.tensor(lam0[b], device=device, requires_grad=True)
        W, sj = pycwt_amd.cwt_torch(xb, DT_T, **kw(name))[:2]
        yb = pycwt_amd.icwt_shrink_torch(W, sj, DT_T, lb, DJ_T, mother_of(name), mode)
        cb = c[b] if batch else c
        (yb * cb).sum().real.backward() if yb.is_complex() else (yb * cb).sum().backward()
        for got, ref in ((y[b] if batch else y, yb), (xt.grad[b] if batch else xt.grad, xb.grad), (lam_t.grad[b] if batch else lam_t.grad, lb.grad)):
            assert same_bits(got.detach().cpu().numpy(), ref.detach().cpu().numpy()), (name, mode, b)
    # lam of shape (rows,) and scale of shape (): autograd sums over the batch
    per_signal = lam_t.grad.detach().reshape(nb, rows).cpu().numpy().astype(np.float64)
    shared = torch.tensor(lam0[0], device=device, requires_grad=True)
    x2 = torch.tensor(xs, device=device, requires_grad=True)
    y2 = pycwt_amd.denoise_torch(x2, DT_T, threshold=shared, mode=mode, **kw(name))[0]
    (y2 * c).sum().real.backward() if y2.is_complex() else (y2 * c).sum().backward()
    assert shared.grad.shape == (rows,)
    if nb == 1:
        assert same_bits(shared.grad.cpu().numpy(), per_signal[0].astype(real))
    scale = torch.tensor(0.9, dtype=torch.float64, device=device, requires_grad=True)
    x3 = torch.tensor(xs, device=device, requires_grad=True)
    y3, lam3 = pycwt_amd.denoise_torch(x3, DT_T, scale=scale, mode=mode, **kw(name))[:2]
    (y3 * c).sum().real.backward() if y3.is_complex() else (y3 * c).sum().backward()
    assert scale.grad.shape == () and bool(torch.isfinite(scale.grad)) and x3.grad.shape == x3.shape
    # d/d scale = sum over signals and rows of (d/d lam) lam / scale: the same thresholds given as a tensor
    given = lam3.detach().clone().requires_grad_(True)
    x4 = torch.tensor(xs, device=device)
    y4 = pycwt_amd.denoise_torch(x4, DT_T, threshold=given, mode=mode, **kw(name))[0]
    (y4 * c).sum().real.backward() if y4.is_complex() else (y4 * c).sum().backward()
    assert same_bits(y4.detach().cpu().numpy(), y3.detach().cpu().numpy())
    want = float((given.grad.double() * lam3.detach() / 0.9).sum())
    mag = float((given.grad.double() * lam3.detach() / 0.9).abs().sum())
    assert abs(float(scale.grad) - want) <= 4 * nb * rows * eps * mag + 0.0, (float(scale.grad), want)
    if mode == "hard":
        assert float(scale.grad) == 0


def check_w_grad_is_the_export(torch, device, lib, prec, mode):
    """icwt_shrink_torch's W.grad = the export's G for the cotangent it received, bit for bit; lam.grad = glambda rounded to lam's type"""
    import pycwt_amd
    real, cplx, eps = types(prec)
    W, sj, lam, gy, _ = inputs(7, 300, prec, "mixed")
    Wt = torch.tensor(W, device=device, requires_grad=True)
    lt = torch.tensor(lam, device=device, requires_grad=True)
    c = torch.tensor(gy, device=device)
    y = pycwt_amd.icwt_shrink_torch(Wt, sj, DT_T, lt, DJ_T, "morlet", mode)
    assert y.dtype == c.dtype and y.shape == (300,)
    y.backward(c)
    coeff = DJ_T * np.sqrt(DT_T) / (mother_of("morlet").cdelta * mother_of("morlet").psi(0))
    g_total = (c * float(np.real(coeff))).cpu().numpy()
    with Dev(lib, 512, prec, max_rows=64) as dev:
        G, gl = run_adjoint(dev, W, sj, lam, mode, g_total, coeff=1.0)
    assert same_bits(Wt.grad.cpu().numpy(), G) and same_bits(lt.grad.cpu().numpy(), gl.astype(real))


def gradcheck_inputs(seed=2, rows=5, ncols=48):
    """(W, sj, lam): |W| at least 10 % away from lam in every entry, so that a probe step of 1e-6 in any component of W or lam moves
    no entry across its threshold: the kept mask is the same at both ends of every probe step (asserted)"""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.3, 3.0, size=(rows, ncols))
    lam = rng.uniform(0.8, 1.2, size=rows)
    ratio = mag / lam[:, None]
    mag = np.where(np.abs(ratio - 1) < 0.15, mag * 1.4, mag)
    W = mag * np.exp(2j * np.pi * rng.random((rows, ncols)))
    step = 1e-6
    margin = np.abs(np.abs(W) - lam[:, None])
    assert np.all(margin >= 0.1 * lam[:, None]) and margin.min() > 4 * step       # |d|W|| <= step, |d lam| <= step
    assert ((np.abs(W) > lam[:, None]).mean() > 0.2) and ((np.abs(W) < lam[:, None]).mean() > 0.05)
    return W, SJ[:rows].copy(), lam, step


def check_gradcheck(torch, device):
    import pycwt_amd
    W, sj, lam, step = gradcheck_inputs()
    Wt = torch.tensor(W, device=device, requires_grad=True)
    lt = torch.tensor(lam, device=device, requires_grad=True)
    assert torch.autograd.gradcheck(lambda w: pycwt_amd.icwt_torch(w, sj, DT_T, DJ_T, "morlet"), (Wt,), eps=step)
    assert torch.autograd.gradcheck(lambda w: pycwt_amd.icwt_torch(w, sj, DT_T, DJ_T, "dog"), (torch.stack([Wt, 2 * Wt]).detach().requires_grad_(True),), eps=step)
    for mode in ("soft", "garrote"):
        assert torch.autograd.gradcheck(lambda w, l: pycwt_amd.icwt_shrink_torch(w, sj, DT_T, l, DJ_T, "morlet", mode), (Wt, lt), eps=step), mode
    lt.grad = None
    pycwt_amd.icwt_shrink_torch(Wt, sj, DT_T, lt, DJ_T, "morlet", "hard").sum().backward()
    assert bool((lt.grad == 0).all())                                # hard: exactly 0
    scalar = torch.tensor(1.0, dtype=torch.float64, device=device, requires_grad=True)
    both = torch.stack([Wt.detach(), 0.5 * Wt.detach()]).requires_grad_(True)
    mask = np.abs(np.abs(np.stack([W, 0.5 * W])) - 1.0)
    assert mask.min() > 4 * step
    assert torch.autograd.gradcheck(lambda w, l: pycwt_amd.icwt_shrink_torch(w, sj, DT_T, l, DJ_T, "paul", "soft"), (both, scalar), eps=step)


def check_central_difference(torch, device, mode="soft", seeds=range(8)):
    """one central difference of denoise_torch along a random direction of x in fp64 with the thresholds given, at a point where
    the kept mask of W(x - h dx), W(x) and W(x + h dx) is the same (the first seed for which it is; asserted to exist).  Each
    evaluation of the loss sum c y is accurate to TOL[64] D sum |c| at worst (the engine's round-off tolerance relative to
    D = |coeff| sum_j max_n |W_j| / sqrt(s_j), shrink_common), so their difference over 2 h is within TOL D sum |c| / h; the
    curvature term of the soft rule is of relative size (h |dW| / |W|)^2 = 1e-10 and is covered by the factor 2."""
    import pycwt_amd
    name = "morlet"
    x = signals(None, 64).astype(np.float64)
    lam = np.linspace(0.05, 0.5, J_T + 1)
    lt = torch.tensor(lam, device=device)
    for seed in seeds:
        rng = np.random.default_rng(seed)
        dx = rng.standard_normal(N0_T)
        c = rng.standard_normal(N0_T)
        h = 1e-5 * np.linalg.norm(x) / np.linalg.norm(dx)
        Ws = [pycwt_amd.cwt_torch(torch.tensor(x + s * h * dx, device=device), DT_T, **kw(name))[0].cpu().numpy() for s in (-1, 0, 1)]
        masks = [np.abs(w) > lam[:, None] for w in Ws]
        if np.array_equal(masks[0], masks[1]) and np.array_equal(masks[1], masks[2]):
            break
    else:
        raise AssertionError("no seed keeps the mask")
    sj = pycwt_amd.cwt_torch(torch.tensor(x, device=device), DT_T, **kw(name))[1]
    ct = torch.tensor(c, device=device)
    xt = torch.tensor(x, device=device, requires_grad=True)
    (pycwt_amd.denoise_torch(xt, DT_T, threshold=lt, mode=mode, **kw(name))[0] * ct).sum().backward()
    an = float((xt.grad.cpu().numpy().astype(L) * dx.astype(L)).sum())
    loss = [float((pycwt_amd.denoise_torch(torch.tensor(x + s * h * dx, device=device), DT_T, threshold=lt, mode=mode, **kw(name))[0] * ct).sum())
            for s in (-1, 1)]
    fd = (loss[1] - loss[0]) / (2 * h)
    m = mother_of(name)
    D = abs(DJ_T * np.sqrt(DT_T) / (m.cdelta * m.psi(0))) * (np.abs(Ws[1]).max(axis=1) / np.sqrt(sj)).sum()
    bound = 2 * TOL[64] * D * np.abs(c).sum() / h
    print(f"central difference {fd:.12e}, gradient {an:.12e}, error {abs(fd - an):.3e}, bound {bound:.3e}")
    assert abs(an) > 0
    assert abs(fd - an) <= bound, (fd, an, bound)


def check_torch_refusals(torch, device):
    import pycwt_amd
    import pytest
    x = torch.tensor(signals(None, 64), device=device)
    W = torch.zeros((4, 32), dtype=torch.complex128, device=device)
    sj = SJ[:4]

    class Duck:
        def psi_ft(self, f):
            return pycwt_amd.Morlet(6).psi_ft(f)

        def flambda(self):
            return pycwt_amd.Morlet(6).flambda()

        def coi(self):
            return pycwt_amd.Morlet(6).coi()
    with pytest.raises(ValueError, match="mode"):
        pycwt_amd.denoise_torch(x, 1.0, mode="firm")
    with pytest.raises(ValueError, match="threshold"):
        pycwt_amd.denoise_torch(x, 1.0, threshold="sure")
    with pytest.raises((NotImplementedError, ValueError, TypeError)):
        pycwt_amd.denoise_torch(x, 1.0, wavelet=Duck())
    with pytest.raises(ValueError):
        pycwt_amd.denoise_torch(x, 1.0, noise_columns=(5, 5))
    with pytest.raises(ValueError):
        pycwt_amd.denoise_torch(x, 1.0, noise_columns=(0, N0_T + 1))
    with pytest.raises(ValueError):
        pycwt_amd.denoise_torch(x, 1.0, threshold=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        pycwt_amd.denoise_torch(x, 1.0, scale=torch.ones((2, 3), dtype=torch.float64))
    with pytest.raises(TypeError):
        pycwt_amd.denoise_torch(x.cpu().numpy(), 1.0)
    with pytest.raises(ValueError):
        pycwt_amd.denoise_torch(x[None, None], 1.0)
    with pytest.raises(TypeError):
        pycwt_amd.denoise_torch(x, 1.0, hop=2)
    with pytest.raises(ValueError, match="mode"):
        pycwt_amd.icwt_shrink_torch(W, sj, 1.0, torch.tensor(0.5), mode="firm")
    with pytest.raises(ValueError):
        pycwt_amd.icwt_shrink_torch(W, sj[:3], 1.0, torch.tensor(0.5))
    with pytest.raises(ValueError):
        pycwt_amd.icwt_shrink_torch(W, sj, 1.0, torch.zeros(3))
    with pytest.raises(ValueError):
        pycwt_amd.icwt_shrink_torch(W, sj, 1.0, torch.zeros((2, 4)))             # (B, rows) needs a batch
    with pytest.raises(ValueError):
        pycwt_amd.icwt_torch(W.real, sj, 1.0)
    with pytest.raises((NotImplementedError, ValueError, TypeError)):
        pycwt_amd.icwt_torch(W, sj, 1.0, wavelet=Duck())


def check_nonfinite_signal(torch, device):
    """a non-finite sample: NaN in that signal's y and gradients; the other signal of the batch as alone"""
    import pycwt_amd
    xs = signals(2, 64)
    xs[0, 17] = np.inf
    lam = torch.tensor(np.full((2, J_T + 1), 0.2), device=device, requires_grad=True)
    xt = torch.tensor(xs, device=device, requires_grad=True)
    y = pycwt_amd.denoise_torch(xt, DT_T, threshold=lam, **kw("morlet"))[0]
    y.abs().sum().backward()
    x1 = torch.tensor(xs[1], device=device, requires_grad=True)
    l1 = torch.tensor(np.full(J_T + 1, 0.2), device=device, requires_grad=True)
    y1 = pycwt_amd.denoise_torch(x1, DT_T, threshold=l1, **kw("morlet"))[0]
    y1.abs().sum().backward()
    assert torch.isnan(y[0]).all() and torch.isnan(xt.grad[0]).all() and torch.isnan(lam.grad[0]).all()
    assert torch.equal(y[1], y1) and torch.equal(xt.grad[1], x1.grad) and torch.equal(lam.grad[1], l1.grad)
    yu, lu = pycwt_amd.denoise_torch(xt.detach(), DT_T, **kw("morlet"))[:2]
    assert torch.isnan(yu[0]).all() and torch.isnan(lu[0]).all() and bool(torch.isfinite(yu[1]).all())


def check_torch_memory(torch, device, rows=32, n0=1 << 15):
    """after denoise_torch's forward, y alive, the node holds nothing of W's size: memory_allocated grows by less than rows x n0 x 8
    bytes (W is rows x n0 x 16 in fp64); icwt_shrink_torch after cwt_torch does hold W, so the measure can tell"""
    import pycwt_amd
    x = torch.tensor(np.random.default_rng(3).standard_normal(n0), device=device, requires_grad=True)
    lam = torch.full((rows,), 0.5, dtype=torch.float64, device=device, requires_grad=True)
    args = dict(dj=1 / 2, J=rows - 1, wavelet="morlet")
    pycwt_amd.denoise_torch(x, 1.0, threshold=lam, **args)[0].sum().backward()          # (the engine exists, the caches are warm)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(device)
    y = pycwt_amd.denoise_torch(x, 1.0, threshold=lam, **args)[0]
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated(device) - before
    assert y.grad_fn is not None and 0 < grown < rows * n0 * 8, grown
    y.sum().backward()
    del y
    before = torch.cuda.memory_allocated(device)
    W, sj = pycwt_amd.cwt_torch(x, 1.0, **args)[:2]
    y = pycwt_amd.icwt_shrink_torch(W, sj, 1.0, lam, args["dj"])
    del W
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(device) - before
    assert held >= rows * n0 * 16, held
    print(f"denoise_torch holds {grown} bytes, cwt_torch -> icwt_shrink_torch {held} (W: {rows * n0 * 16})")


def check_torch_stream(torch, device):
    """forward and backward on a stream that is not the default one, back to back without a host synchronisation in between:
    the bits of the same on the default stream"""
    import pycwt_amd
    x = signals(None, 64)
    rng = np.random.default_rng(62)
    c = torch.tensor(rng.standard_normal(N0_T), device=device)
    lam0 = np.linspace(0.05, 0.5, J_T + 1)

    def run():
        xt = torch.tensor(x, device=device, requires_grad=True)
        lt = torch.tensor(lam0, device=device, requires_grad=True)
        y = pycwt_amd.denoise_torch(xt, DT_T, threshold=lt, mode="garrote", **kw("morlet"))[0]
        (y * c).sum().backward()
        W, sj = pycwt_amd.cwt_torch(xt.detach(), DT_T, **kw("morlet"))[:2]
        W.requires_grad_(True)
        (pycwt_amd.icwt_torch(W, sj, DT_T, DJ_T) * c).sum().backward()
        return y.detach(), xt.grad, lt.grad, W.grad
    base = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):
        first = run()
        second = run()
    side.synchronize()
    for got in (first, second):
        assert all(torch.equal(a, b) for a, b in zip(base, got))
    run()                                                           # and back on the default stream
    torch.cuda.synchronize()


def check_large(lib, mode):
    """3 rows x (2^17 + 3) columns, one row over 65 slices: the closed form in both precisions, and the fp32 gradient against the fp64
    run of the same (fp32) inputs at fp32 round-off -- the bounds of fp32 plus those of fp64"""
    nrows, ncols = LARGE
    W, sj, lam, gy, _ = inputs(nrows, ncols, 32, "mixed")
    got = {}
    for prec in PRECS:
        real, cplx, eps = types(prec)
        with Dev(lib, 16, prec, max_rows=16) as dev:
            G, gl = run_adjoint(dev, W.astype(cplx), sj, lam.astype(real), mode, gy.astype(real))
        compare(G, gl, W.astype(cplx), sj, lam.astype(real), mode, COEFF, gy.astype(real), eps)
        got[prec] = (G, gl)
    e32, e64 = types(32)[2], types(64)[2]
    tabs = reference(W, sj, lam, mode, COEFF, gy)[3]
    terms = np.abs(reference(W, sj, lam, mode, COEFF, gy)[2]).sum(axis=1)
    u = (G_BOUND[mode] + 2) * L(e32) / 2 + G_BOUND[mode] * L(e64) / 2                # (+ 2: T(coeff) and w_j rounded to fp32 or not)
    d = got[32][0].astype(np.complex128) - got[64][0]
    assert np.all(np.maximum(np.abs(d.real), np.abs(d.imag)).astype(L) <= u * tabs)
    ul = (glambda_bound_units(mode, ncols, e32) + 2) * L(e32) / 2 + glambda_bound_units(mode, ncols, e64) * L(e64) / 2
    assert np.all(np.abs(got[32][1] - got[64][1]).astype(L) <= ul * terms)
