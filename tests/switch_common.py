"""Shared by test_switch_scales_emulated.py, test_switch_scales_gpu.py and tests/perf/switch_scales.py: the scales at which the
row classifier (plan_host.cpp: row_support, poly_candidate, ols_candidate, classify_row, aols_pass) changes its mind, and the
transform at those scales against the oracle.

A switch is a pair of ADJACENT doubles (s_lo, s_hi = nextafter(s_lo, inf)) that the classifier gives two different labels.  The
pairs are found through the classifier under test (find_switches: Plan.classify on a geometric probe grid, then bisection with
one-scale calls), so that they follow every retuning of a threshold; what the kernels compute there is judged by the oracle
alone.  These are the worst rows of the accuracy contract -- a polynomial row at the highest degree its K' allows, an
overlap-save row with the least slack under its halo rounding, a row that only just counts as not clipped at Nyquist -- and the
capability limits of the forms sit on them (nband exactly K, t1 == narrow_terms, halo exactly a quarter tile).

FAMILIES holds, per (log2 N -- which fixes the options --, precision, mother, target, entry point), the families of switches that
the search found on the CPU emulation (checked, not assumed: written by tests/perf/switch_scales.py --families).  A retuning that removes a family fails
assert_families and edits the list in its own change instead of testing less in silence.
"""
import functools

import numpy as np

from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import FORMS_OPTS

MOTHERS = [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2), (orc.DOG, 3)]
SENTINEL = -7.0
ALPHA = -0.75
PROBES = 3000
MAX_ROWS = 4096          # of the plans: the probe grid is classified in one call (the row tables are all that grows with it)
# (log2 N, plan options): the smallest transform that has every row form; the smallest at which the production gates
# ols_min_logn / poly_min_logn are the ones in force; the flagship length of bench.py (GPU only)
SIZES = {15: FORMS_OPTS, 18: None, 20: None}
N0_OFF = 77
TARGETS = {64: [0.0, 1e-12, 1e-9, 1e-7, 1e-6], 32: [0.0, 3e-5]}          # 0: round-off
BENCH = {64: 1e-9, 32: 3e-5}
FLAGSHIP_ROWS = 64       # pair rows per call at N = 2^20: W is 1 GiB at most


def value_cases(logn):
    """(log2 N, precision, mother, parameter, target, signal): both signals at round-off and at the bench target"""
    out = []
    for prec in (64, 32):
        for kind, param in MOTHERS:
            for target in TARGETS[prec]:
                out.append((logn, prec, kind, param, target, "white"))
                if target in (0.0, BENCH[prec]):
                    out.append((logn, prec, kind, param, target, "impulses"))
    return out


def rows_cases():
    """the spectrum-only entry point: 2^15 at round-off and at the bench target, 2^18 at the bench target"""
    return [(logn, prec, kind, param, target, "white") for logn in (15, 18) for prec in (64, 32) for kind, param in MOTHERS
            for target in ((0.0, BENCH[prec]) if logn == 15 else (BENCH[prec],))]


def flagship_cases():
    """N = 2^20 with the default options, where the classifier runs as bench.py runs it (GPU only)"""
    return [(20, prec, kind, param, target, "white") for prec, kind, param in ((64, orc.MORLET, 6), (32, orc.DOG, 2))
            for target in (0.0, BENCH[prec])]


def case_id(c):
    return "2^%d-fp%d-%s-%g-%s" % (c[0], c[1], mother_id(c[2], c[3]), c[4], c[5])


def types(prec):
    return (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)


def mother_id(kind, param):
    return "%s%g" % (["morlet", "paul", "dog"][kind], param)


def probe_grid(n0, m, probes=PROBES):
    """geometric, from the Fourier period 2 dt to n0 dt (dt = 1), without the rows that the reference turns into NaN"""
    s0 = 2.0 / m.flambda()
    sj = s0 * (n0 / 2.0) ** (np.arange(probes) / (probes - 1.0))
    return sj[~orc.dropped_rows(sj, 1.0, m)]


def find_switches(plan, kind, param, n0, ncols, with_signal, probes=PROBES):
    """[(s_lo, s_hi, label_lo, label_hi)] with s_hi == nextafter(s_lo, inf): every adjacent pair of the probe grid that
    Plan.classify -- one call over the whole grid, as a real call sees its rows -- labels differently, bisected with one-scale
    calls until the two scales are adjacent doubles.  The labels are those of the one-scale calls; the band-passed form is decided
    per call over all rows, so a probe pair that a row alone does not tell apart is no switch, and a switch of the rows alone
    that the grid call hides under that form is one if it holds in the call of the pairs (below).  Where the reference drops
    the largest scales (Paul), the largest scale it keeps is a probe too.  Sorted by scale."""
    m = orc.Mother(kind, param)
    sj = probe_grid(n0, m, probes)
    s0 = 2.0 / m.flambda()
    if len(sj) < probes:                                   # (dropped_rows keeps a grid that is dropped whole: ask with s0)
        def dropped(s):
            return bool(orc.dropped_rows(np.array([s0, s]), 1.0, m)[1])
        lo, hi = float(sj[-1]), float(s0 * (n0 / 2.0) ** (len(sj) / (probes - 1.0)))
        assert not dropped(lo) and dropped(hi)
        while np.nextafter(lo, np.inf) < hi:
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if dropped(mid) else (mid, hi)
        if lo > sj[-1]:
            sj = np.append(sj, lo)
    labels = plan.classify(kind, param, 1.0, sj, ncols, with_signal)

    def one(s):
        return plan.classify(kind, param, 1.0, [s], ncols, with_signal)[0]

    def bisect(lo, hi, la, lb, into):
        while np.nextafter(lo, np.inf) < hi:
            mid = 0.5 * (lo + hi)
            lm = one(mid)
            if lm == la:
                lo = mid
            elif lm == lb:
                hi = mid
            else:                                   # a third label in between: two switches (or more) in this probe step
                bisect(lo, mid, la, lm, into)
                lo, la = mid, lm
        into.append((lo, hi, la, lb))
    out = []
    for i in np.flatnonzero([a != b for a, b in zip(labels[:-1], labels[1:])]):
        lo, hi = float(sj[i]), float(sj[i + 1])
        la, lb = one(lo), one(hi)
        if la != lb:
            bisect(lo, hi, la, lb, out)
    # Switches under the band-passed form.  A call over the whole range moves its clipped and wide rows to that form ('aols',
    # decided per call), and the grid call then shows one label where the rows alone have two.  The call of the pairs is no call
    # over the whole range: such a switch is a pair too if it straddles TOGETHER with the pairs found so far and costs none of
    # them its own straddling (tried from the smallest scale up, each kept or dropped for good).
    hidden = []
    # (every 8th probe of a stretch with one label of that form, and its last: the supports shrink with the scale, so these
    # switches come in one order, and a one-scale call of such a row costs its halo search)
    i = 0
    while i < len(labels):
        j = i
        while j + 1 < len(labels) and labels[j + 1] == labels[i]:
            j += 1
        if labels[i].startswith("aols"):
            at = sorted(set(range(i, j + 1, 8)) | {j})
            alone = [one(float(sj[k])) for k in at]
            for a, b, la, lb in zip(at[:-1], at[1:], alone[:-1], alone[1:]):
                if la != lb:
                    bisect(float(sj[a]), float(sj[b]), la, lb, hidden)
        i = j + 1

    def straddling(pairs):
        lab = plan.classify(kind, param, 1.0, pair_scales(pairs), ncols, with_signal)
        return [lab[2 * k] != lab[2 * k + 1] for k in range(len(pairs))]
    for h in hidden:
        trial = sorted(out + [h])
        before, after = straddling(out) if out else [], straddling(trial)
        k = trial.index(h)
        if after[k] and after[:k] + after[k + 1:] == before:
            out = trial
    return sorted(out)


def family(label_lo, label_hi):
    """The form (the label up to the first '/') on either side; where the form stays, the names of the parts that change:
    ('ols', 'narrow'), ('poly/d', 'poly/d'), ('poly/K/d', 'poly/K/d'), ('ols/K/half', 'ols/K/-'), ('two_pass/full', 'two_pass/c')."""
    a, b = label_lo.split("/"), label_hi.split("/")
    if a[0] != b[0]:
        return a[0], b[0]
    keep = [i for i in range(1, max(len(a), len(b))) if (a[i:i + 1] != b[i:i + 1])]
    return tuple("/".join([p[0]] + [p[i].rstrip("0123456789") if i < len(p) else "-" for i in keep]) for p in (a, b))


def signal(name, n0, prec, seed=3):
    """rounded to the precision under test; the oracle sees the same numbers"""
    real = types(prec)[0]
    if name == "white":
        return np.random.default_rng(seed).standard_normal(n0).astype(real)
    assert name == "impulses", name
    x = np.zeros(n0, dtype=real)           # the wavelet itself at block and tile edges: where a short halo shows
    for i, v in ((0, 1.0), (4096, -2.5), (8191, 0.75), (n0 // 3, -1.5), (n0 - 1, 3.0)):
        if i < n0:
            x[i] = v
    return x


def draw_q(shape, real, seed=21):
    """weights of the weighted output: both signs, about 1 % exact zeros"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal(shape)
    Q[rng.random(shape) < 0.01] = 0.0
    return Q.astype(real)


def pair_scales(pairs):
    return np.array([s for p in pairs for s in p[:2]], dtype=np.float64)


def thin(pairs, most):
    """at most `most` pairs: pairs of families already represented go first, never the last of a family"""
    pairs = list(pairs)
    while len(pairs) > most:
        fams = [family(p[2], p[3]) for p in pairs]
        count = {f: fams.count(f) for f in fams}
        f = max(count, key=lambda k: (count[k], k))
        assert count[f] > 1, "more families than rows allowed"
        del pairs[max(i for i, g in enumerate(fams) if g == f)]
    return pairs


_found = {}


class Result:
    """what run_pairs returns: W (rows x n0), the row classes of the call, the pairs, the oracle's rows and their peaks, and the
    per-row error max|dW| / peak; with extras the other outputs of the same plan"""

    def worst(self):
        j = int(np.argmax(self.err))
        return float(self.sj[j]), self.classes[j], float(self.err[j])

    def straddling(self):
        """indices of the pairs whose two rows still carry different labels after the call"""
        return [i for i in range(len(self.pairs)) if self.classes[2 * i] != self.classes[2 * i + 1]]


def row_error(W, ref, peak):
    """per row max|dW| / peak (row by row: the rows of N = 2^20 are 16 MiB each)"""
    d = np.array([np.abs(w.astype(np.complex128) - r).max() for w, r in zip(np.asarray(W), ref)])
    return d / np.where(peak == 0, 1.0, peak)


def run_pairs(lib, N, n0, prec, kind, param, opts, target, signal_name, extras=(), with_signal=True, most=None, adjoint_poly=None):
    """One cwt_transform (with_signal = False: forward_fft + cwt_transform_rows) over the scales of every switch pair, in pair
    order, on one plan at the accuracy target (0 = round-off); the switches are found on that plan after set_tolerance, since
    they move with the target.  extras: "power", "weighted" (the sibling calls on the same plan), "adjoint" (cwt_adjoint_rows
    with the pair scales after the forward: the cached table; G is seeded noise, gives .G and .xbar)."""
    real, cplx = types(prec)
    m = orc.Mother(kind, param)
    options = dict(opts or {})
    if adjoint_poly is not None:
        options["adjoint_poly"] = adjoint_poly
    plan = _hip.Plan(N, prec, max_rows=MAX_ROWS, lib=lib, options=options)
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        b = _hip.DeviceBuffer(max(a.nbytes, 16), lib=lib)
        bufs.append(b)
        b.upload(plan, a)
        return b
    r = Result()
    try:
        plan.set_tolerance(target)
        # (the search depends on the library, the plan's shape, options and target alone: the signals, the extras and the other
        # entry points of a case share it)
        key = (id(lib), N, n0, prec, kind, param, tuple(sorted(options.items())), target, with_signal)
        if key not in _found:
            _found[key] = find_switches(plan, kind, param, n0, n0, with_signal)
        pairs = list(_found[key])
        if most is not None:
            pairs = thin(pairs, most)
        r.pairs, r.sj = pairs, pair_scales(pairs)
        rows = len(r.sj)
        assert 0 < rows <= plan.max_rows, rows
        x = signal(signal_name, n0, prec)
        xd, xh = up(x), up(np.zeros(N, dtype=cplx))
        Wd = up(np.zeros((rows, n0), dtype=cplx))
        if with_signal:
            plan.transform(xd.ptr, n0, kind, param, 1.0, r.sj, xh.ptr, Wd.ptr, n0, n0)
        else:
            plan.forward_fft(xd.ptr, n0, xh.ptr)
            plan.transform_rows(xh.ptr, kind, param, 1.0, r.sj, Wd.ptr, n0, n0)
        r.classes = plan.row_classes()
        r.W = Wd.download(plan, (rows, n0), cplx)
        if "power" in extras:
            Pd = up(np.full((rows, n0), SENTINEL, dtype=real))
            plan.transform_power(xd.ptr, n0, kind, param, 1.0, r.sj, xh.ptr, Pd.ptr, n0, n0)
            assert plan.row_classes() == r.classes
            r.P = Pd.download(plan, (rows, n0), real)
        if "weighted" in extras:
            r.Q = draw_q((rows, n0), real)
            Qd, Gd = up(r.Q), up(np.full((rows, n0), SENTINEL * (1 + 1j), dtype=cplx))
            plan.transform_weighted(xd.ptr, n0, kind, param, 1.0, r.sj, xh.ptr, Qd.ptr, ALPHA, Gd.ptr, n0, n0)
            assert plan.row_classes() == r.classes
            r.Gw = Gd.download(plan, (rows, n0), cplx)
        if "adjoint" in extras:
            rng = np.random.default_rng(11)
            r.G = (rng.standard_normal((rows, n0)) + 1j * rng.standard_normal((rows, n0))).astype(cplx)
            Ad, xb = up(r.G), up(np.zeros(n0, dtype=real))
            plan.adjoint_rows(Ad.ptr, 1, rows * n0, n0, n0, kind, param, 1.0, r.sj, xb.ptr, n0)
            r.xbar = xb.download(plan, (n0,), real)
    finally:
        for b in bufs:
            b.free()
        plan.close()
    r.x = x
    r.ref = oracle_rows(N, n0, prec, kind, param, signal_name, tuple(r.sj))
    r.peak = np.abs(r.ref).max(axis=1)
    r.err = row_error(r.W, r.ref, r.peak)
    return r


@functools.lru_cache(maxsize=4)
def oracle_rows(N, n0, prec, kind, param, signal_name, sj):
    """the oracle's rows of the case's signal at transform length N, trimmed to n0: read-only"""
    x = signal(signal_name, n0, prec).astype(np.float64)
    W = orc.cwt_rows(x, 1.0, np.array(sj), orc.Mother(kind, param), N=N)[:, :n0]
    W.flags.writeable = False
    return W


def assert_straddling(r, need=4):
    """Condition, not measurement: the band-passed form is decided per call over all rows, so a pair may legitimately stop
    straddling in the real call -- at most one pair in ten of a case, and the rest number at least `need`."""
    keep = r.straddling()
    lost = len(r.pairs) - len(keep)
    assert lost * 10 <= len(r.pairs), (lost, len(r.pairs), r.classes)
    assert len(keep) >= need, (len(keep), r.classes)
    return keep


def families_of(r, keep=None):
    keep = range(len(r.pairs)) if keep is None else keep
    return {family(r.classes[2 * i], r.classes[2 * i + 1]) for i in keep}


def family_errors(r, keep):
    """{family: the larger error of the worst pair of it}"""
    out = {}
    for i in keep:
        f = family(r.classes[2 * i], r.classes[2 * i + 1])
        out[f] = max(out.get(f, 0.0), float(r.err[2 * i]), float(r.err[2 * i + 1]))
    return out


# ---- the shapes of section E: cwt_transform with ncols != n0 and ldw > ncols -------------------------------------------------
def shapes(N):
    """(n0, ncols, ldw)"""
    return [(N - 77, 10001, 10007), (N // 2 + 333, N, N), (N, N // 2 + 1, N // 2 + 9), (N - 77, N, N + 3), (5000, N - 1, N),
            (N - 77, 1, 5), (N - 77, 8192, 8192), (N - 77, 4033, 4033)]


def run_shape(lib, N, prec, kind, param, opts, shape, power=False, grid_rows=40):
    """cwt_transform (power: cwt_transform_power) of n0 samples writing ncols columns on a leading dimension ldw, at round-off:
    a grid_rows grid over the whole range plus the case's switch pairs.  Returns the whole rows x ldw matrix (prefilled with
    SENTINEL), the row classes, the scales, the oracle's first ncols columns (transform length N, a signal of n0 samples)
    and the peak of every oracle row."""
    n0, ncols, ldw = shape
    real, cplx = types(prec)
    m = orc.Mother(kind, param)
    plan = _hip.Plan(N, prec, max_rows=MAX_ROWS, lib=lib, options=dict(opts or {}))
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        b = _hip.DeviceBuffer(max(a.nbytes, 16), lib=lib)
        bufs.append(b)
        b.upload(plan, a)
        return b
    try:
        key = (id(lib), N, n0, ncols, prec, kind, param, tuple(sorted((opts or {}).items())))
        if key not in _found:                          # (the complex and the power output of a shape share the search)
            _found[key] = find_switches(plan, kind, param, n0, ncols, True)
        pairs = _found[key]
        sj = np.concatenate([probe_grid(n0, m, grid_rows), pair_scales(pairs)])
        rows = len(sj)
        assert rows <= plan.max_rows, rows
        x = signal("white", n0, prec)
        xd, xh = up(x), up(np.zeros(N, dtype=cplx))
        if power:
            od = up(np.full((rows, ldw), SENTINEL, dtype=real))
            plan.transform_power(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, od.ptr, ldw, ncols)
            out = od.download(plan, (rows, ldw), real)
        else:
            od = up(np.full((rows, ldw), SENTINEL * (1 + 1j), dtype=cplx))
            plan.transform(xd.ptr, n0, kind, param, 1.0, sj, xh.ptr, od.ptr, ldw, ncols)
            out = od.download(plan, (rows, ldw), cplx)
        classes = plan.row_classes()
    finally:
        for b in bufs:
            b.free()
        plan.close()
    ref = orc.cwt_rows(x.astype(np.float64), 1.0, sj, m, N=N)
    peak = np.abs(ref[:, :max(n0, ncols)]).max(axis=1)          # the row's peak, not that of the ncols columns asked for
    return out, classes, sj, ref[:, :ncols], peak


# ---- the families that must occur --------------------------------------------------------------------------------------------
# key: (log2 N, precision, mother, target, with the signal); written by tests/perf/switch_scales.py --families on the CPU emulation
FAMILIES = {
    (15, 64, 'morlet6', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'morlet6', 1e-12, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'morlet6', 1e-09, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 64, 'morlet6', 1e-07, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'morlet6', 1e-06, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'paul4', 0.0, True): {
        ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass',
        'narrow_k2048'), ('two_pass/full', 'two_pass/c')},
    (15, 64, 'paul4', 1e-12, True): {
        ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass',
        'narrow_k2048'), ('two_pass/full', 'two_pass/c')},
    (15, 64, 'paul4', 1e-09, True): {
        ('aols', 'narrow_k2048'), ('aols', 'two_pass'), ('aols/P', 'aols/P'), ('narrow/t', 'narrow/-'), ('narrow/t',
        'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'aols')},
    (15, 64, 'paul4', 1e-07, True): {
        ('aols', 'ols'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t',
        'narrow_k2048/t'), ('ols', 'narrow_k2048'), ('ols/K', 'ols/K')},
    (15, 64, 'paul4', 1e-06, True): {
        ('aols', 'ols'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('ols',
        'narrow_k2048'), ('ols/K', 'ols/K'), ('ols/K/half', 'ols/K/-')},
    (15, 64, 'dog2', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog2', 1e-12, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog2', 1e-09, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog2', 1e-07, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 64, 'dog2', 1e-06, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog3', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog3', 1e-12, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog3', 1e-09, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 64, 'dog3', 1e-07, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 64, 'dog3', 1e-06, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d')},
    (15, 32, 'morlet6', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 32, 'morlet6', 3e-05, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 32, 'paul4', 0.0, True): {
        ('aols', 'ols'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('ols', 'narrow'), ('ols/K', 'ols/K'),
        ('ols/K/half', 'ols/K/-')},
    (15, 32, 'paul4', 3e-05, True): {
        ('aols', 'ols'), ('narrow/t', 'narrow/-'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('ols/K/half', 'ols/K/-')},
    (15, 32, 'dog2', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 32, 'dog2', 3e-05, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 32, 'dog3', 0.0, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (15, 32, 'dog3', 3e-05, True): {
        ('aols', 'ols'), ('narrow', 'poly'), ('ols', 'narrow'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d',
        'poly/d')},
    (18, 64, 'morlet6', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'morlet6', 1e-12, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'morlet6', 1e-09, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'morlet6', 1e-07, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'morlet6', 1e-06, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'paul4', 0.0, True): {
        ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'narrow_k2048'), ('two_pass/c', 'two_pass/c'), ('two_pass/full',
        'two_pass/c')},
    (18, 64, 'paul4', 1e-12, True): {
        ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'narrow_k2048'), ('two_pass/c', 'two_pass/c'), ('two_pass/full',
        'two_pass/c')},
    (18, 64, 'paul4', 1e-09, True): {
        ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'narrow_k2048'), ('two_pass/c', 'two_pass/c')},
    (18, 64, 'paul4', 1e-07, True): {
        ('aols', 'narrow_k2048'), ('aols', 'ols'), ('narrow_k2048/t', 'narrow_k2048/t'), ('ols', 'aols'), ('ols/K', 'ols/K')},
    (18, 64, 'paul4', 1e-06, True): {
        ('aols', 'narrow_k2048'), ('aols', 'ols'), ('narrow_k2048/t', 'narrow_k2048/t'), ('ols', 'aols'), ('ols/K', 'ols/K'),
        ('ols/K/half', 'ols/K/-')},
    (18, 64, 'dog2', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog2', 1e-12, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog2', 1e-09, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog2', 1e-07, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'dog2', 1e-06, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'dog3', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog3', 1e-12, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog3', 1e-09, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (18, 64, 'dog3', 1e-07, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 64, 'dog3', 1e-06, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'morlet6', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'morlet6', 3e-05, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'paul4', 0.0, True): {
        ('narrow/t', 'narrow/t'), ('ols', 'two_pass'), ('ols/K', 'ols/K'), ('ols/K/half', 'ols/K/-'), ('ols2', 'two_pass'),
        ('two_pass', 'narrow'), ('two_pass', 'ols'), ('two_pass', 'ols2')},
    (18, 32, 'paul4', 3e-05, True): {
        ('ols', 'ols2'), ('ols/K', 'ols/K'), ('ols/K/half', 'ols/K/-'), ('ols2', 'narrow'), ('ols2/K', 'ols2/K'), ('two_pass',
        'ols')},
    (18, 32, 'dog2', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'dog2', 3e-05, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'dog3', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (18, 32, 'dog3', 3e-05, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (15, 64, 'morlet6', 0.0, False): {
        ('aols', 'two_pass'), ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048',
        'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'narrow_k2048'), ('two_pass/full', 'two_pass/c')},
    (15, 64, 'morlet6', 1e-09, False): {
        ('aols', 'two_pass'), ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048',
        'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass',
        'narrow_k2048'), ('two_pass/full', 'two_pass/c')},
    (15, 64, 'paul4', 0.0, False): {
        ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass',
        'narrow_k2048'), ('two_pass/full', 'two_pass/c')},
    (15, 64, 'paul4', 1e-09, False): {
        ('aols', 'narrow_k2048'), ('aols', 'two_pass'), ('aols/P', 'aols/P'), ('narrow/t', 'narrow/-'), ('narrow/t',
        'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'aols')},
    (15, 64, 'dog2', 0.0, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t',
        'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'narrow_k2048'), ('two_pass/full',
        'two_pass/c')},
    (15, 64, 'dog2', 1e-09, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t',
        'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'narrow_k2048'), ('two_pass/full',
        'two_pass/c')},
    (15, 64, 'dog3', 0.0, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t',
        'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'narrow_k2048'), ('two_pass/full',
        'two_pass/c')},
    (15, 64, 'dog3', 1e-09, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('narrow_k2048', 'narrow'), ('narrow_k2048/t',
        'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass', 'narrow_k2048'), ('two_pass/full',
        'two_pass/c')},
    (15, 32, 'morlet6', 0.0, False): {
        ('aols', 'two_pass'), ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'),
        ('poly/d', 'poly/d'), ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (15, 32, 'morlet6', 3e-05, False): {
        ('aols', 'two_pass'), ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'),
        ('poly/d', 'poly/d'), ('two_pass', 'narrow')},
    (15, 32, 'paul4', 0.0, False): {
        ('aols', 'two_pass'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('two_pass', 'narrow'), ('two_pass/full',
        'two_pass/c')},
    (15, 32, 'paul4', 3e-05, False): {
        ('aols', 'narrow'), ('aols', 'two_pass'), ('aols/P', 'aols/P'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t')},
    (15, 32, 'dog2', 0.0, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'),
        ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (15, 32, 'dog2', 3e-05, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'),
        ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (15, 32, 'dog3', 0.0, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'),
        ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (15, 32, 'dog3', 3e-05, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/-'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'),
        ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (18, 64, 'morlet6', 1e-09, False): {
        ('narrow_k2048', 'poly'), ('narrow_k2048/t', 'narrow_k2048/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'),
        ('two_pass', 'narrow_k2048'), ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (18, 64, 'paul4', 1e-09, False): {
        ('narrow_k2048/t', 'narrow_k2048/t'), ('two_pass', 'narrow_k2048'), ('two_pass/c', 'two_pass/c')},
    (18, 64, 'dog2', 1e-09, False): {
        ('narrow_k2048', 'poly'), ('narrow_k2048/t', 'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'narrow_k2048'), ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (18, 64, 'dog3', 1e-09, False): {
        ('narrow_k2048', 'poly'), ('narrow_k2048/t', 'narrow_k2048/t'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'narrow_k2048'), ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (18, 32, 'morlet6', 3e-05, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'narrow'),
        ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (18, 32, 'paul4', 3e-05, False): {
        ('narrow/t', 'narrow/t'), ('two_pass', 'narrow'), ('two_pass/full', 'two_pass/c')},
    (18, 32, 'dog2', 3e-05, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'narrow'),
        ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (18, 32, 'dog3', 3e-05, False): {
        ('narrow', 'poly'), ('narrow/t', 'narrow/t'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'narrow'),
        ('two_pass/c', 'two_pass/c'), ('two_pass/full', 'two_pass/c')},
    (20, 64, 'morlet6', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('ols/half', 'ols/-'), ('poly/K', 'poly/K'), ('poly/d', 'poly/d'), ('two_pass',
        'ols')},
    (20, 64, 'morlet6', 1e-09, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (20, 32, 'dog2', 0.0, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
    (20, 32, 'dog2', 3e-05, True): {
        ('ols', 'poly'), ('ols/K', 'ols/K'), ('poly/K/d', 'poly/K/d'), ('poly/d', 'poly/d'), ('two_pass', 'ols')},
}


def assert_families(key, have):
    want = FAMILIES[key]
    assert want, key
    assert want <= have, (key, sorted(want - have), sorted(have))
