"""Shared by tests/test_pool_emulated.py, tests/test_pool_gpu.py and tests/perf/pool_accuracy.py: the cases of the time-pooled
scalogram (cwt_transform_pool), its references and its bounds.

Primary reference: the SAME plan's cwt_transform_power output (same options, tolerance and signal), pooled on the host in long
double by the definition -- Pbar[j, m] = the mean of |W[j, n]|^2 over the columns of window m inside [0, n0).  The two paths share
every truncation, down to the same coefficient planes; they differ by rounding and the order of summation only.  Per row,
max_m |Pbar - ref| / max_m ref.  The bound is MEASURED, not chosen (profiles/pool_accuracy.txt, written by
tests/perf/pool_accuracy.py on the CPU emulation): the worst ratio over the emulated cases below is MEASURED[precision], and the
tests assert 4 x that (FMA contraction and the GPU's instruction order; the order of summation itself is fixed by design).  A
measured value above 256 eps would be a defect in the summation, not a bound to adopt (asserted below).

Second, independent reference: the oracle (oracle/cwt_oracle.py), pooled the same way, per row relative to the row's peak power,
within 2 x the round-off tolerance of tests/test_gpu_parity.py (1e-11 / 3e-5 on W; d|W|^2 = 2 |W| d|W|).
"""
import numpy as np

from oracle import cwt_oracle as orc
from hop_common import Device, types
from poly_xcd_common import IDX, TOLERANCE as POLY_TOLERANCE, WANT, kd_of, scales as poly_scales
from test_kernels_emulated import grid
from test_power_emulated import FORMS

# worst per-row ratio over the emulated cases (every form x pools, the (K', D) rows at 1e-9 and at round-off, the short signal),
# per precision: profiles/pool_accuracy.txt
MEASURED = {64: 4.564e-16, 32: 2.741e-07}
BOUND = {p: 4 * e for p, e in MEASURED.items()}
for _p, _e in MEASURED.items():
    assert _e <= 256 * float(np.finfo(types(_p)[0]).eps), "a defect in the summation, not a bound"
ORACLE_BOUND = {64: 2 * 1e-11, 32: 2 * 3e-5}          # 2 x TOL of tests/test_gpu_parity.py

FORM_POOLS = (2, 64, 4096)
NFFT_POOL_FORMS = ("ols", "poly")                     # pool = nfft (one window per row) on these two
POLY_POOLS = (16, 128, 1024)
SENTINEL = -7.0


def form_pools(form):
    """the pools of one FORMS entry: {2, 64, 4096} where pool <= nfft, and pool = nfft (one window per row) on two of the forms"""
    return [h for h in FORM_POOLS if h <= form[1]] + ([form[1]] if form[0] in NFFT_POOL_FORMS else [])


def window_means(P, h):
    """rows x n0 -> rows x ceil(n0 / h) in long double, by the definition"""
    P = np.asarray(P).astype(np.longdouble)
    rows, n0 = P.shape
    nc = -(-n0 // h)
    out = np.empty((rows, nc), dtype=np.longdouble)
    full = (n0 // h) * h
    if full:
        out[:, :n0 // h] = P[:, :full].reshape(rows, -1, h).sum(axis=2) / h
    if full < n0:
        out[:, -1] = P[:, full:].sum(axis=1) / (n0 - full)
    return out


def row_ratio(got, ref):
    """per row max_m |got - ref| / max_m ref"""
    got = np.asarray(got).astype(np.longdouble)
    return np.asarray(np.abs(got - ref).max(axis=1) / ref.max(axis=1), dtype=np.float64)


def run_power(dev, x, kind, param, sj):
    """cwt_transform_power of one signal: rows x n0 reals"""
    x = np.asarray(x, dtype=dev.real)
    n0 = x.size
    xd, Pd = dev.up(x), dev.up(np.zeros((len(sj), n0), dtype=dev.real))
    dev.plan.transform_power(xd.ptr, n0, kind, param, 1.0, sj, None, Pd.ptr, n0, n0)
    return Pd.download(dev.plan, (len(sj), n0), dev.real)


def run_pool(dev, x, kind, param, sj, pool, ld_pad=0, extra_rows=0, xhat=None):
    """cwt_transform_pool of x ((n0,) or (nb, n0)): the whole (nb * rows + extra_rows) x (ceil(n0 / pool) + ld_pad) matrix,
    prefilled with SENTINEL"""
    x = np.atleast_2d(np.asarray(x, dtype=dev.real))
    nb, n0 = x.shape
    ld = -(-n0 // pool) + ld_pad
    shape = (nb * len(sj) + extra_rows, ld)
    out, xd = dev.up(np.full(shape, SENTINEL, dtype=dev.real)), dev.up(x)
    dev.plan.transform_pool(xd.ptr, nb, n0, n0, kind, param, 1.0, sj, pool, xhat.ptr if xhat is not None else None, out.ptr, ld)
    return out.download(dev.plan, shape, dev.real)


def form_signal(n0):
    return np.random.default_rng(7).standard_normal(n0)


def check_form(lib, form, prec, bound=None):
    """One (form, precision) case, every pool of form_pools on ONE plan: the form carries rows, each pooled call classifies as
    the power call of that plan, padding columns and extra rows keep the sentinel; returns {pool: worst per-row ratio against the
    pooled power of the same plan} (each asserted <= bound if given)."""
    name, N, n0, kind, param, rows, opts, want = form
    want = want[prec] if isinstance(want, dict) else want
    x = form_signal(n0)
    sj = grid(n0, 1.0, orc.Mother(kind, param), rows)
    errs = {}
    with Device(lib, N, prec, max_rows=len(sj), options=opts) as dev:
        P = run_power(dev, x, kind, param, sj)
        split = dev.plan.last_split()
        assert split[want] > 0, split
        for pool in form_pools(form):
            nc = -(-n0 // pool)
            B = run_pool(dev, x, kind, param, sj, pool, ld_pad=3, extra_rows=2)
            assert dev.plan.last_split() == split
            assert np.all(B[:len(sj), nc:] == SENTINEL) and np.all(B[len(sj):] == SENTINEL)
            errs[pool] = err = row_ratio(B[:len(sj), :nc], window_means(P, pool)).max()
            print("pooled rows against the pooled power:", name, "pool", pool, "precision", prec, err, "bound", bound)
            if bound is not None:
                assert err <= bound, (name, pool, err, bound)
    return errs


def check_poly_rows(lib, prec, tolerance, bound=None, n0=(1 << 16) - 37, want=None):
    """The rows IDX of the 256-scale grid at N = 2^16 (polynomial form), every pool of POLY_POOLS on one plan: pooled against the
    pooled power of the same plan; tolerance 0 = the precision's round-off default.  Returns ({pool: worst ratio}, the (K', D)
    pairs of the rows)."""
    N = 1 << 16
    sj = poly_scales(N, IDX)
    x = np.random.default_rng(5).standard_normal(n0)
    errs = {}
    with Device(lib, N, prec, max_rows=len(sj), options={"poly_min_logn": 14}) as dev:
        dev.plan.set_tolerance(tolerance)
        P = run_power(dev, x, MORLET, F0, sj)
        classes = dev.plan.row_classes()
        polys = [c for c in classes if c.startswith("poly/")]
        have = {kd_of(c) for c in polys}
        assert polys, classes
        if want is not None:
            assert len(polys) == len(classes) and want <= have, (classes, sorted(want - have))
        for pool in POLY_POOLS:
            B = run_pool(dev, x, MORLET, F0, sj, pool)
            errs[pool] = err = row_ratio(B, window_means(P, pool)).max()
            print("polynomial rows:", sorted(have), "tolerance", tolerance, "pool", pool, "precision", prec, err, "bound", bound)
            if bound is not None:
                assert err <= bound, (pool, err, bound)
    return errs, have


MORLET, F0 = orc.MORLET, 6.0
SHORT = dict(N=1 << 16, n0=(1 << 15) + 1, pool=4096, rows=24)     # exactly 9 windows, the last of one column


def check_short_signal(lib, prec, bound=None):
    N, n0, pool = SHORT["N"], SHORT["n0"], SHORT["pool"]
    sj = grid(n0, 1.0, orc.Mother(MORLET, F0), SHORT["rows"])
    x = np.random.default_rng(19).standard_normal(n0)
    with Device(lib, N, prec, max_rows=len(sj), options={"poly_min_logn": 14, "ols_min_logn": 15}) as dev:
        P = run_power(dev, x, MORLET, F0, sj)
        B = run_pool(dev, x, MORLET, F0, sj, pool, ld_pad=2)
    assert -(-n0 // pool) == 9 and np.all(B[:, 9:] == SENTINEL)
    last = row_ratio(B[:, 8:9], P[:, -1:].astype(np.longdouble)).max()      # the last window is the last column itself
    err = max(row_ratio(B[:, :9], window_means(P, pool)).max(), 0.0)
    print("short signal: precision", prec, err, "last window", last, "bound", bound)
    if bound is not None:
        assert err <= bound and last <= bound, (err, last, bound)
    return err


def oracle_case(prec):
    """(N, n0, sj, x, per-pool oracle window means) of one Morlet case for the independent check"""
    N, n0 = 1 << 15, (1 << 15) - 77
    sj = grid(n0, 1.0, orc.Mother(MORLET, F0), 40)
    x = np.random.default_rng(29).standard_normal(n0).astype(types(prec)[0])
    W = orc.cwt_rows(x.astype(np.float64), 1.0, sj, orc.Mother(MORLET, F0), N=N)[:, :n0]
    return N, n0, sj, x, W.real ** 2 + W.imag ** 2
