"""Shared by tests/test_shrink_emulated.py, tests/test_shrink_gpu.py, tests/test_shrink_schedules_emulated.py and
tests/perf/denoise_accuracy.py: the cases, references and bounds of wavelet shrinkage -- cwt_row_order_statistics,
cwt_icwt_shrink (include/cwt_hip.h) and the shim around them (row_quantiles, noise_levels, icwt_shrink, denoise).

SELECTION, REAL INPUT: equality with np.sort(row)[rank] (NaN matches NaN; np.sort puts every NaN last, as the kernel's keys do).
SELECTION, COMPLEX INPUT: the reference v = re^2 + im^2 is formed in long double and the kernel's v = fma(re, re, im im) differs
from it by rounding.  Two checks per (row, rank):
  value    |out - s| <= 2 ulp, s = the reference's order statistic rounded to the plan's precision T (one rounding of im im and
           one of the fma: 1.5 ulp).  The rounding to T is where a value beyond T's range becomes inf or 0 for the kernel too.
  bracket  #{v_ref < out (1 - 4 eps)} <= rank < #{v_ref <= out (1 + 4 eps)}: the rank of `out` among the reference's values is
           right up to the entries within rounding of it.  The relative margin is meaningless below T's normal range and at inf,
           so v_ref is first passed through T's range (beyond the largest finite: inf) and the margin is never smaller than two of
           T's smallest denormal; in the normal range this is the formula as written.
SHRINK-INVERSE: the reference shrinks the plan's own W in long double by the definitions of include/cwt_hip.h and sums it in long
double; the error of a signal is max_n |out - ref| / D with D = |coeff| sum_j max_n |W_j| / sqrt(s_j).  The bound is MEASURED:
tests/perf/denoise_accuracy.py runs CASES on the emulation and writes the worst error per precision, in units of eps, to
profiles/denoise_accuracy.txt; the tests assert 4 x that (fused multiply-adds and the GPU's instruction order are not the
emulation's).  A measured value above 256 eps would be a defect of the summation (133 rows in 8 partial sums: about 17 additions
per sum), not a bound to adopt: asserted here at import.
The hard rule is discontinuous, so `thresholds` places lambda_j^2 at the geometric mean of the two adjacent order statistics of
v with the widest ratio among the ranks n / 4 ... 3 n / 4 of the row and asserts that ratio >= 1 + 128 eps: no entry is within
rounding of its threshold (a row of one column has no pair: lambda^2 = v / 4).
"""
import ctypes as C
import os

import numpy as np

from conftest import ROOT
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from ssq_common import Dev, EINVAL, PRECS, launch_log, padded, types  # noqa: F401  (re-exported to the test modules)

L = np.longdouble
SENTINEL = -7.0
PAD = 5                                   # ld = ncols + PAD, the padding NaN
MODES = ("hard", "soft", "garrote")
ACCURACY_FILE = os.path.join(ROOT, "profiles", "denoise_accuracy.txt")


def read_measured(path=ACCURACY_FILE):
    """{precision: worst error of CASES on the emulation, in eps}; empty until tests/perf/denoise_accuracy.py has written it"""
    out = {}
    if os.path.exists(path):
        for line in open(path):
            f = line.split()
            if len(f) >= 3 and f[0] in ("fp64", "fp32") and f[1] == "worst_error_in_eps":
                out[int(f[0][2:])] = float(f[2])
    return out


MEASURED = read_measured()
assert all(0 < v <= 256 for v in MEASURED.values()), MEASURED     # above: a defect in the summation, not a bound to adopt


def shrink_bound(prec):
    assert prec in MEASURED, f"{ACCURACY_FILE} has no fp{prec} line: run tests/perf/denoise_accuracy.py"
    return 4 * MEASURED[prec] * types(prec)[2]


# ---- selection: rows ---------------------------------------------------------------------------------------------------------------
KINDS = ("gauss", "constant", "two_values", "ties90", "magnitudes", "signs_zeros", "one_inf", "nans")


def adversarial_row(kind, ncols, prec, rng):
    """(row, ranks of its own): the rank on either side of a boundary where the row has one"""
    real = types(prec)[0]
    fi = np.finfo(real)
    n = ncols
    own = []
    if kind == "gauss":
        row = rng.standard_normal(n)
    elif kind == "constant":
        row = np.full(n, 1.25)
    elif kind == "two_values":                                   # 1 : 999, the rank on either side of the boundary
        a = max(1, -(-n // 1000))
        row = np.where(rng.permutation(n) < a, -3.0, 0.1)
        own = [a - 1, a]
    elif kind == "ties90":                                       # 90 % one value, the rest in its binade: one first digit
        row = np.where(rng.random(n) < 0.9, 1.5, rng.uniform(1.0, 2.0, n))
    elif kind == "magnitudes":                                   # the smallest denormal ... the largest finite
        lo, hi = int(np.log2(float(fi.smallest_subnormal))), int(fi.maxexp) - 1
        row = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(lo, hi + 1, n)).astype(real)
        row[rng.integers(n)] = fi.smallest_subnormal
        row[rng.integers(n)] = fi.max
        row[np.isinf(row)] = fi.max
    elif kind == "signs_zeros":
        row = rng.standard_normal(n)
        z = rng.random(n)
        row[z < 0.1] = 0.0
        row[z > 0.9] = -0.0
        own = [int((row < 0).sum()), int((row <= 0).sum()) - 1, int((row <= 0).sum())]
    elif kind == "one_inf":
        row = rng.standard_normal(n)
        row[rng.integers(n)] = np.inf
    elif kind == "nans":                                         # 5 % NaN of both sign bits, ranks on both sides of the count
        row = rng.standard_normal(n).astype(real)
        where = rng.permutation(n)[:max(1, n // 20)]
        row[where[0::2]] = np.nan
        row[where[1::2]] = -np.nan
        bits = row.view(np.uint64 if prec == 64 else np.uint32)
        bits[where[1::2]] |= np.array(1, dtype=bits.dtype) << (bits.dtype.itemsize * 8 - 1)
        cnt = n - where.size
        own = [cnt - 1, cnt]
    else:
        raise KeyError(kind)
    return np.asarray(row, dtype=real), [r for r in own if 0 <= r < n]


def selection_matrix(nrows, ncols, prec, seed, first_kind=0):
    """nrows rows, row j of kind (first_kind + j) mod 8; the ranks of the case: 0, ncols - 1, the two middle ranks, five seeded ones
    and the rows' own"""
    rng = np.random.default_rng([seed, nrows, ncols, prec])
    rows, ranks = [], [0, ncols - 1, (ncols - 1) // 2, ncols // 2] + rng.integers(0, ncols, 5).tolist()
    for j in range(nrows):
        row, own = adversarial_row(KINDS[(first_kind + j) % len(KINDS)], ncols, prec, rng)
        rows.append(row)
        ranks += own
    return np.stack(rows), np.unique(np.array(ranks, dtype=np.int64))


NCOLS = (1, 2, 255, 256, 257, 4099)
# (nrows, ncols, first kind): three rows at every size, the kinds taken in turn (every kind at every size); one row of every kind
# at 257 columns.  On the GPU also 300 rows at 257 columns and rows that span workgroups.
SELECT_CASES = [(3, n, k) for n in NCOLS for k in (0, 3, 6)] + [(1, 257, k) for k in range(len(KINDS))]
SELECT_CASES_GPU = [(300, 257, 0), (600, 257, 0)] + [(3, (1 << 17) + 3, k) for k in (0, 3, 6)]    # (600 rows x 8 ranks: two slabs of scratch)


def run_select(dev, A, ranks, is_complex):
    """cwt_row_order_statistics on A with ld = ncols + PAD (the padding NaN), at most 8 ranks per call, into an out of nrows + 1
    rows and nranks + 2 columns prefilled with the sentinel; returns nrows x len(ranks)"""
    nrows, ncols = A.shape
    nan = complex(np.nan, np.nan) if is_complex else np.nan
    Ad = dev.up(padded(A, PAD, nan))
    got = np.empty((nrows, len(ranks)), dtype=dev.real)
    for i in range(0, len(ranks), 8):
        part = np.asarray(ranks[i:i + 8], dtype=np.int64)
        ldo = part.size + 2
        od = dev.up(np.full((nrows + 1, ldo), SENTINEL, dtype=dev.real))
        dev.plan.row_order_statistics(Ad.ptr, is_complex, ncols + PAD, ncols, nrows, part, od.ptr, ldo)
        out = od.download(dev.plan, (nrows + 1, ldo), dev.real)
        assert np.all(out[:, part.size:] == SENTINEL) and np.all(out[nrows] == SENTINEL)        # beyond nranks, beyond nrows
        got[:, i:i + part.size] = out[:nrows, :part.size]
    assert np.array_equal(Ad.download(dev.plan, (nrows, ncols + PAD), A.dtype).view(np.uint8), padded(A, PAD, nan).view(np.uint8))   # inputs are inputs
    dev.release()
    return got


def same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def check_select_real(dev, nrows, ncols, first_kind, seed=11):
    A, ranks = selection_matrix(nrows, ncols, dev.prec, seed, first_kind)
    got = run_select(dev, A, ranks, False)
    want = np.sort(A, axis=1)[:, ranks]
    ok = same(got, want)
    assert ok.all(), (np.argwhere(~ok)[:4].tolist(), got[~ok][:4], want[~ok][:4])


def assert_complex_statistics(got, Wc, ranks, prec):
    """the two checks of a complex selection (module docstring); got: nrows x len(ranks) of the plan's precision"""
    real, _, eps = types(prec)
    fi = np.finfo(real)
    with np.errstate(all="ignore"):
        v = Wc.real.astype(L) ** 2 + Wc.imag.astype(L) ** 2
        v_t = np.where(v > L(fi.max), L(np.inf), v)                     # through T's range (NaN stays NaN)
        stat = np.sort(v, axis=1)[:, ranks].astype(real)
        tiny = L(fi.smallest_subnormal)
        for j in range(Wc.shape[0]):
            for i, r in enumerate(ranks):
                out, s = got[j, i], stat[j, i]
                if np.isnan(s) or np.isnan(out):
                    assert np.isnan(s) and np.isnan(out), (j, r, out, s)
                    continue
                assert out == s or abs(L(out) - L(s)) <= 2 * L(np.spacing(np.abs(s))), (j, r, out, s)
                margin = max(4 * L(eps) * abs(L(out)), 2 * tiny) if np.isfinite(out) else L(0)
                below, upto = int((v_t[j] < L(out) - margin).sum()), int((v_t[j] <= L(out) + margin).sum())
                assert below <= r < upto, (j, r, out, below, upto)


def check_select_complex_rows(dev, nrows, ncols, first_kind, seed=12):
    """the adversarial rows fed as (re, 0)"""
    A, ranks = selection_matrix(nrows, ncols, dev.prec, seed, first_kind)
    Wc = A.astype(dev.cplx)
    assert_complex_statistics(run_select(dev, Wc, ranks, True), Wc, ranks, dev.prec)


# ---- a real W: Morlet, n0 = 4099 on N = 8192, 133 scales from 2 dt on --------------------------------------------------------------
N0, NFFT, ROWS_W = 4099, 8192, 133
SJ = 2.0 * 2.0 ** (np.arange(ROWS_W) / 12.0)
_w_cache = {}


def transform_once(plan, x, sj, real, cplx):
    """W (rows x N0, the plan's precision) of one cwt_transform on this plan"""
    xd = _hip.DeviceBuffer(N0 * np.dtype(real).itemsize, lib=plan.lib)
    Wd = _hip.DeviceBuffer(sj.size * N0 * np.dtype(cplx).itemsize, lib=plan.lib)
    try:
        xd.upload(plan, x.astype(real))
        plan.transform(xd.ptr, N0, orc.MORLET, 6.0, 1.0, sj, None, Wd.ptr, N0, N0)
        return Wd.download(plan, (sj.size, N0), cplx)
    finally:
        xd.free()
        Wd.free()


def noise_signal(seed=5):
    return np.random.default_rng(seed).standard_normal(N0)


def real_w(lib, prec):
    """the W of Gaussian noise that the selection and shrink cases run on, computed once per library and precision"""
    key = (id(lib), prec)
    if key not in _w_cache:
        with Dev(lib, NFFT, prec, max_rows=ROWS_W) as dev:
            _w_cache[key] = transform_once(dev.plan, noise_signal(), SJ, dev.real, dev.cplx)
        _w_cache[key].flags.writeable = False
    return _w_cache[key]


def check_select_complex_w(dev, rows=slice(0, ROWS_W, 11)):
    Wc = np.ascontiguousarray(real_w(dev.lib, dev.prec)[rows])
    rng = np.random.default_rng(3)
    ranks = np.unique(np.array([0, N0 - 1, (N0 - 1) // 2, N0 // 2] + rng.integers(0, N0, 5).tolist()))
    assert_complex_statistics(run_select(dev, Wc, ranks, True), Wc, ranks, dev.prec)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def refusals(dev, nrows=3, ncols=257):
    """(label, return code) of every argument set the two entry points refuse, and whether every buffer kept its bits"""
    rng = np.random.default_rng(4)
    Wc = (rng.standard_normal((nrows, ncols)) + 1j * rng.standard_normal((nrows, ncols))).astype(dev.cplx)
    ld = ncols + PAD
    Wp = padded(Wc, PAD, 0)
    start = np.full((nrows + 1, 16), SENTINEL, dtype=dev.real)
    vec = np.full(ncols + PAD, SENTINEL, dtype=dev.real)
    lam = np.zeros(nrows, dtype=dev.real)
    Wd, od, vd, ld_dev = dev.up(Wp), dev.up(start), dev.up(vec), dev.up(lam)
    lib, h, P = dev.lib, dev.plan.h, C.c_void_p
    sj = np.arange(1.0, nrows + 1)
    sp = sj.ctypes.data_as(C.POINTER(C.c_double))

    def select(A=Wd.ptr, cplx=1, ld=ld, ncols=ncols, nrows=nrows, ranks=(0, 1), nranks=None, out=od.ptr, ldo=16, plan=h):
        r = np.array(ranks if len(ranks) else [0], dtype=np.int64)
        rp = None if ranks is None else r.ctypes.data_as(C.POINTER(C.c_int64))
        return lib.cwt_row_order_statistics(plan, P(A), cplx, ld, ncols, nrows, rp, len(ranks) if nranks is None else nranks, P(out), ldo)

    def shrink(W=Wd.ptr, ldw=ld, ncols=ncols, nrows=nrows, s=sp, lam=ld_dev.ptr, mode=1, out=vd.ptr, plan=h):
        return lib.cwt_icwt_shrink(plan, P(W), ldw, ncols, nrows, s, P(lam), mode, 1.0, P(out))

    bad = np.array([1.0, 0.0, 3.0][:nrows])
    out = [("nranks 0", select(ranks=(), nranks=0)), ("nranks 9", select(ranks=tuple(range(9)))), ("rank -1", select(ranks=(0, -1))),
           ("rank ncols", select(ranks=(ncols,))), ("ncols 0", select(ncols=0, ranks=(0,))), ("nrows 0", select(nrows=0)),
           ("ld < ncols", select(ld=ncols - 1)), ("ldo < nranks", select(ldo=1)), ("is_complex 2", select(cplx=2)),
           ("A NULL", select(A=None)), ("out NULL", select(out=None)), ("select plan NULL", select(plan=None)),
           ("mode 3", shrink(mode=3)), ("mode -1", shrink(mode=-1)), ("shrink ncols 0", shrink(ncols=0)), ("shrink nrows 0", shrink(nrows=0)),
           ("nrows > max_rows", shrink(nrows=dev.plan.max_rows + 1)), ("ldw < ncols", shrink(ldw=ncols - 1)),
           ("scale 0", shrink(s=bad.ctypes.data_as(C.POINTER(C.c_double)))), ("W NULL", shrink(W=None)), ("lambda NULL", shrink(lam=None)),
           ("out NULL", shrink(out=None)), ("scales NULL", shrink(s=None)), ("shrink plan NULL", shrink(plan=None))]
    dev.plan.sync()
    untouched = (np.array_equal(od.download(dev.plan, start.shape, dev.real), start) and np.array_equal(vd.download(dev.plan, vec.shape, dev.real), vec)
                 and np.array_equal(Wd.download(dev.plan, Wp.shape, dev.cplx), Wp))
    dev.release()
    return out, untouched


# ---- shrink-inverse ----------------------------------------------------------------------------------------------------------------
SHRINK_ROWS, SHRINK_NCOLS = (1, 7, 8, 9, 133), (1, 127, 128, 129, 4099)
COEFF = 0.37
# (nrows, ncols, pattern of lambda): "mixed" at every shape; every lambda 0 and every lambda +inf at every row count
CASES = [(r, n, "mixed") for r in SHRINK_ROWS for n in SHRINK_NCOLS] + [(r, 129, p) for r in SHRINK_ROWS for p in ("zero", "inf")]


def abs2_long(Wc):
    return Wc.real.astype(L) ** 2 + Wc.imag.astype(L) ** 2


def thresholds(Wc, prec, pattern):
    """lambda per row, of the plan's precision: "zero", "inf", or "mixed" = between two well separated order statistics of the row
    (module docstring), with every fifth row 0 and every seventh +inf"""
    real, _, eps = types(prec)
    nrows, n = Wc.shape
    if pattern == "zero":
        return np.zeros(nrows, dtype=real)
    if pattern == "inf":
        return np.full(nrows, np.inf, dtype=real)
    v = np.sort(abs2_long(Wc), axis=1)
    lam = np.empty(nrows, dtype=real)
    for j in range(nrows):
        if n == 1:
            lam2 = v[j, 0] / 4
        else:
            lo = n // 4
            hi = max(lo + 1, min(n - 1, (3 * n) // 4))
            ratio = v[j, lo + 1:hi + 1] / v[j, lo:hi]
            i = int(np.argmax(ratio))
            assert ratio[i] >= 1 + 128 * eps, (j, float(ratio[i]))
            lam2 = np.sqrt(v[j, lo + i] * v[j, lo + i + 1])
        lam[j] = real(np.sqrt(lam2))
    lam[3::5] = 0
    lam[5::7] = np.inf
    return lam


def shrink_reference(Wc, sj, lam, mode, coeff):
    """(ref, D) in long double by the definitions of include/cwt_hip.h"""
    re, v = Wc.real.astype(L), abs2_long(Wc)
    lm = lam.astype(L)[:, None]
    with np.errstate(all="ignore"):
        if mode == "hard":
            f = np.where(v > lm * lm, L(1), L(0))
        elif mode == "soft":
            f = np.maximum(0, 1 - lm / np.sqrt(v))
        else:
            f = np.maximum(0, 1 - lm * lm / v)
        f = np.where((v == 0) | np.isinf(lm), L(0), f)
    w = 1 / np.sqrt(sj.astype(L))[:, None]
    ref = L(coeff) * (re * f * w).sum(axis=0)
    D = abs(L(coeff)) * (np.abs(Wc).astype(L).max(axis=1) / np.sqrt(sj.astype(L))).sum()
    return ref, D


def run_shrink(dev, Wc, sj, lam, mode, coeff=COEFF, reduce_too=False):
    """cwt_icwt_shrink with ldw = ncols + PAD (the padding NaN) into an out prefilled with the sentinel behind ncols; with
    reduce_too also cwt_icwt_reduce of the same arguments"""
    nrows, ncols = Wc.shape
    Wd = dev.up(padded(Wc, PAD, complex(np.nan, np.nan)))
    ld_dev = dev.up(lam)
    od = dev.up(np.full(ncols + 2, SENTINEL, dtype=dev.real))
    dev.plan.icwt_shrink(Wd.ptr, ncols + PAD, ncols, sj, ld_dev.ptr, mode, coeff, od.ptr)
    out = od.download(dev.plan, (ncols + 2,), dev.real)
    assert np.all(out[ncols:] == SENTINEL)
    if reduce_too:
        dev.plan.icwt_reduce(Wd.ptr, ncols + PAD, ncols, sj, coeff, od.ptr)
        red = od.download(dev.plan, (ncols,), dev.real)
        dev.release()
        return out[:ncols], red
    dev.release()
    return out[:ncols]


def shrink_error(dev, nrows, ncols, pattern, mode):
    """max_n |out - ref| / D of one case, in units of eps"""
    Wc = np.ascontiguousarray(real_w(dev.lib, dev.prec)[:nrows, :ncols])
    sj = SJ[:nrows]
    lam = thresholds(Wc, dev.prec, pattern)
    out = run_shrink(dev, Wc, sj, lam, mode)
    ref, D = shrink_reference(Wc, sj, lam, mode, COEFF)
    if pattern == "inf":
        assert np.all(out == 0)
    return float(np.abs(out.astype(L) - ref).max() / D / L(dev.eps))


def check_shrink(dev, nrows, ncols, pattern, mode):
    err = shrink_error(dev, nrows, ncols, pattern, mode)
    print(f"fp{dev.prec} {nrows} x {ncols} {pattern} {mode}: {err:.3f} eps (bound {shrink_bound(dev.prec) / dev.eps:.3f})")
    assert err * dev.eps <= shrink_bound(dev.prec), (nrows, ncols, pattern, mode, err)


def check_special_entries(dev):
    """v = 0 gives 0, lambda = 0 keeps everything, lambda = +inf drops the row, a NaN entry propagates -- to its column alone"""
    rng = np.random.default_rng(9)
    Wc = (rng.standard_normal((4, 6)) + 1j * rng.standard_normal((4, 6))).astype(dev.cplx)
    Wc[1, 2] = 0
    Wc[2, 4] = complex(1.0, np.nan)
    sj = np.array([1.0, 2.0, 4.0, 8.0])
    for mode in MODES:
        lam = np.array([0.0, 0.5, 0.0, np.inf], dtype=dev.real)
        out = run_shrink(dev, Wc, sj, lam, mode, coeff=1.0)
        assert np.isnan(out[4]) and np.isfinite(np.delete(out, 4)).all(), (mode, out)
        ok = np.delete(np.arange(6), 4)
        ref, D = shrink_reference(Wc[:, ok], sj, lam, mode, 1.0)
        assert np.abs(out[ok].astype(L) - ref).max() <= 8 * dev.eps * D, mode
        keep = run_shrink(dev, Wc[:, ok], sj, np.zeros(4, dtype=dev.real), mode, coeff=1.0)
        full, _ = shrink_reference(Wc[:, ok], sj, np.zeros(4, dtype=dev.real), "hard", 1.0)
        assert np.abs(keep.astype(L) - full).max() <= 8 * dev.eps * D, mode


def check_bit_identity(dev, nrows, ncols):
    """every lambda = 0 in hard mode: cwt_icwt_reduce bit for bit"""
    Wc = np.ascontiguousarray(real_w(dev.lib, dev.prec)[:nrows, :ncols])
    out, red = run_shrink(dev, Wc, SJ[:nrows], np.zeros(nrows, dtype=dev.real), "hard", reduce_too=True)
    assert np.array_equal(out.view(np.uint8), red.view(np.uint8)), (nrows, ncols)


def check_scratch_reuse(lib, prec):
    """the same two calls on a fresh plan, and after an unrelated transform on the same plan: the same bits"""
    Wc = np.ascontiguousarray(real_w(lib, prec)[:9, :4099])
    rng = np.random.default_rng(6)
    ranks = np.array([0, 2049, 2050, 4098])
    lam = thresholds(Wc, prec, "mixed")
    got = []
    for warm in (False, True):
        with Dev(lib, NFFT, prec, max_rows=ROWS_W) as dev:
            if warm:
                transform_once(dev.plan, rng.standard_normal(N0), SJ[:40] * 1.1, dev.real, dev.cplx)
            a = run_select(dev, Wc, ranks, True)
            if warm:
                transform_once(dev.plan, rng.standard_normal(N0), SJ[:40] * 1.1, dev.real, dev.cplx)
                b = run_select(dev, np.ascontiguousarray(Wc[:2, :300]), np.array([5]), True)         # ... and another selection
                assert np.isfinite(b).all()
            got.append((a, run_shrink(dev, Wc, SJ[:9], lam, "soft"), run_select(dev, Wc, ranks, True)))
    for x, y in zip(*got):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(got[0][0], got[0][2])


def check_live_plan_sequence(lib, prec):
    """transform -> order statistics -> transform on one plan: the second W is the first bit for bit"""
    x = noise_signal(8)
    with Dev(lib, NFFT, prec, max_rows=ROWS_W) as dev:
        W1 = transform_once(dev.plan, x, SJ, dev.real, dev.cplx)
        got = run_select(dev, W1, np.array([0, 2049, 4098]), True)
        W2 = transform_once(dev.plan, x, SJ, dev.real, dev.cplx)
    assert np.array_equal(W1.view(dev.real), W2.view(dev.real)) and np.isfinite(got).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
E2E_MOTHERS = {"morlet": (orc.MORLET, 6.0), "dog": (orc.DOG, 2.0)}
TOL = {64: 1e-11, 32: 3e-5}              # the round-off tolerance of tests/test_gpu_parity.py (tests/test_shrink_gpu.py asserts they agree)
C_COMPLEX, C_REAL = float(np.sqrt(np.log(4.0))), 0.6744897501960817


def soft_numpy(W, lam):
    with np.errstate(all="ignore"):
        f = np.maximum(0, 1 - lam[:, None] / np.abs(W))
    return W * np.where(np.abs(W) == 0, 0, f)


def oracle_pipeline(x, dt, dj, name, mode_fn=soft_numpy, columns=None, scale=1.0):
    """(y_ref, lam_ref, D): the steps of denoise in NumPy on the oracle's W -- np.median of |W|, lambda, the shrink, orc.icwt"""
    kind, param = E2E_MOTHERS[name]
    m = orc.Mother(kind, param)
    W, sj = orc.cwt(x, dt, dj, -1, -1, m)[:2]
    a, b = (0, x.size) if columns is None else columns
    c = C_REAL if kind == orc.DOG else C_COMPLEX
    lam = scale * np.median(np.abs(W[:, a:b]), axis=1) / c * np.sqrt(2 * np.log(x.size))
    y = orc.icwt(mode_fn(W, lam), sj, dt, dj, m)
    coeff = dj * np.sqrt(dt) / (m.cdelta * m.psi0())
    D = abs(coeff) * (np.abs(W).max(axis=1) / np.sqrt(sj)).sum()
    return y, lam, D, W, sj


def check_oracle_parity(name, prec, columns=None):
    import pycwt_amd
    x = noise_signal(21) + np.sin(2 * np.pi * np.arange(N0) / 64.0)
    dt, dj = 0.5, 1 / 6
    y, lam, sj, freqs, coi = pycwt_amd.denoise(x, dt, dj, wavelet=name, mode="soft", noise_columns=columns, precision=prec)
    y_ref, lam_ref, D, _, sj_ref = oracle_pipeline(x, dt, dj, name, columns=columns)
    assert y.shape == y_ref.shape == (N0,) and np.allclose(sj, sj_ref, rtol=1e-14, atol=0)
    err = float(np.abs(y - y_ref).max())
    print(f"fp{prec} {name} columns {columns}: max|y - y_ref| / D = {err / D:.3e} (bound {2 * TOL[prec]:.1e}); "
          f"max rel lambda error {np.abs(lam / lam_ref - 1).max():.3e}")
    assert err <= 2 * TOL[prec] * D, (err, D)


def check_denoise_surface(prec):
    """explicit thresholds as array and scalar; the returned lam; the refusals; row_quantiles of DeviceTransform and DevicePower"""
    import pycwt_amd
    import pytest
    x = noise_signal(22)
    dt, dj = 1.0, 1 / 4
    real = types(prec)[0]
    D = pycwt_amd.cwt_device(x, dt, dj, precision=prec)
    Dh = pycwt_amd.cwt_device(x, dt, dj, precision=prec, hop=4)
    Pw = pycwt_amd.cwt_power_device(x, dt, dj, precision=prec)
    try:
        rows = D.sj.size
        W = D.W().astype(D._plan.cplx)
        sigma = D.noise_levels()
        y, lam, sj, freqs, coi = pycwt_amd.denoise(x, dt, dj, precision=prec, scale=0.8)
        assert np.array_equal(lam, 0.8 * sigma * np.sqrt(2 * np.log(N0))) and np.array_equal(sj, D.sj)
        assert np.array_equal(y, D.icwt_shrink(dj, lam, "soft"))
        lam_rows = np.linspace(0.1, 2.0, rows)
        y2, lam2 = pycwt_amd.denoise(x, dt, dj, precision=prec, threshold=lam_rows, mode="garrote")[:2]
        assert np.array_equal(lam2, lam_rows) and np.array_equal(y2, D.icwt_shrink(dj, lam_rows, "garrote"))
        y3, lam3 = pycwt_amd.denoise(x, dt, dj, precision=prec, threshold=0.7, mode="hard")[:2]
        assert np.array_equal(lam3, np.full(rows, 0.7)) and np.array_equal(y3, D.icwt_shrink(dj, 0.7, "hard"))
        ref, Dn = shrink_reference(W, D.sj, np.full(rows, 0.7, dtype=real), "hard", 1.0)
        coeff = dj * np.sqrt(dt) / (D.mother.cdelta * D.mother.psi(0))
        near = np.abs(np.abs(W) / 0.7 - 1).min(axis=0) < 64 * types(prec)[2]              # columns with an entry within rounding of 0.7
        assert near.sum() <= 2
        assert np.abs(y3 / coeff - ref.astype(np.float64))[~near].max() <= rows * types(prec)[2] * float(Dn)
        assert np.array_equal(pycwt_amd.denoise(x, dt, dj, precision=prec, threshold=0.0, mode="hard")[0], D.icwt(dj))
        # quantiles: the kernel's own order statistics (exact), NumPy's "lower" rule, np.median for q = 0.5
        q = [0.0, 0.25, 0.5, 0.9, 1.0]
        pw = Pw.power().astype(real)
        want = np.stack([np.quantile(pw, qq, axis=1, method="lower") if qq != 0.5 else np.median(pw.astype(np.float64), axis=1) for qq in q], axis=1)
        assert np.array_equal(Pw.row_quantiles(q), want)
        win = (100, 1100)                                                                # an even count: the median averages two
        want = np.median(pw[:, win[0]:win[1]].astype(np.float64), axis=1)
        assert np.array_equal(Pw.row_quantiles(0.5, columns=win)[:, 0], want)
        got = D.row_quantiles(q)
        mod = np.abs(W.astype(np.complex128))
        want = np.stack([np.quantile(mod, qq, axis=1, method="lower") for qq in q], axis=1)
        assert got.shape == (rows, len(q)) and np.abs(got / want - 1).max() <= 4 * types(prec)[2]
        assert np.abs(D.noise_levels(win) * C_COMPLEX / np.median(mod[:, win[0]:win[1]], axis=1) - 1).max() <= 4 * types(prec)[2]
        for bad in ({"columns": (5, 5)}, {"columns": (0, N0 + 1)}, {"q": 1.5}, {"q": -0.1}):
            with pytest.raises(ValueError):
                D.row_quantiles(bad.get("q", 0.5), columns=bad.get("columns"))
        with pytest.raises(ValueError, match="decimated"):
            Dh.icwt_shrink(dj, 0.5)
        with pytest.raises(ValueError, match="mode"):
            D.icwt_shrink(dj, 0.5, "firm")
    finally:
        D.close()
        Dh.close()
        Pw.close()
    with pytest.raises(ValueError, match="real 1-D"):
        pycwt_amd.denoise(np.zeros((2, 64)), 1.0)
    with pytest.raises(ValueError, match="real 1-D"):
        pycwt_amd.denoise(np.zeros(64, dtype=np.complex128), 1.0)
    with pytest.raises(ValueError, match="threshold"):
        pycwt_amd.denoise(x, 1.0, threshold="sure")
    with pytest.raises(ValueError, match="mode"):
        pycwt_amd.denoise(x, 1.0, mode="firm")

    class Duck:
        pass
    with pytest.raises((NotImplementedError, ValueError, TypeError)):
        pycwt_amd.denoise(x, 1.0, wavelet=Duck())
    # a real mother: the other constant
    Dd = pycwt_amd.cwt_device(x, dt, dj, wavelet="dog", precision=prec)
    try:
        mod = np.abs(Dd.W())
        assert np.abs(Dd.noise_levels() * C_REAL / np.median(mod, axis=1) - 1).max() <= 4 * types(prec)[2]
    finally:
        Dd.close()


def chirp_in_noise(seed=7):
    """(x, clean): a Gaussian-windowed chirp plus 0.3 white noise, n0 = 4099"""
    t = np.arange(N0, dtype=np.float64)
    clean = np.exp(-0.5 * ((t - N0 / 2) / (N0 / 8)) ** 2) * np.cos(2 * np.pi * (0.01 * t + 0.5 * (0.04 / N0) * t * t))
    return clean + 0.3 * np.random.default_rng(seed).standard_normal(N0), clean


def check_functional(prec=64):
    """Morlet, hard, dt = 1, dj = 1 / 12, s0 = 2 dt: the rms of y - clean is below half the rms of x - clean (a wrong c or a
    wrong sqrt(2 ln n) fails this where parity against a reference with the same mistake would not)"""
    import pycwt_amd
    x, clean = chirp_in_noise()
    y = pycwt_amd.denoise(x, 1.0, 1 / 12, 2.0, wavelet="morlet", mode="hard", precision=prec)[0]
    rms = lambda a: float(np.sqrt(np.mean(np.abs(a) ** 2)))      # noqa: E731
    before, after = rms(x - clean), rms(np.real(y) - clean)
    print(f"rms(x - clean) = {before:.4f}, rms(y - clean) = {after:.4f}, ratio {after / before:.3f}")
    assert after < 0.5 * before, (after, before)
