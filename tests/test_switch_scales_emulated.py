"""The forward transform at the scales where the row classifier switches (switch_common.py), on the CPU emulation of the HIP
runtime (tests/emu).  Every case finds the switch pairs of its plan (adjacent doubles with two labels), runs them in ONE call
and judges every row against the oracle, relative to the row's own peak.

A  values at every switch pair: N = 2^15 with FORMS_OPTS and 2^18 with the default options, n0 = N - 77, four mothers, both
   precisions, every accuracy target (fp64: round-off, 1e-12, 1e-9, 1e-7, 1e-6; fp32: round-off, 3e-5); white noise, and the
   impulse signal at round-off and at the bench target;  B  the spectrum-only entry point (no overlap-save form there: other
   switches);  C  the power and the weighted output at the pairs, against the W of the same plan;  D  the adjoint at the pairs
   (the cached table of the forward), against the NumPy adjoint and through the adjoint identity;  E  cwt_transform with
   ncols != n0 and ldw > ncols;  F  the pairs through cwt_transform_batch.

Bounds: at round-off test_kernels_emulated.TOL (1e-12 / 2e-5); with a target, the target itself -- README's contract on white
noise -- and max(target, 2e-5) in fp32; C: test_power_emulated.power_bound and test_weighted_emulated.weighted_bound; D:
test_adjoint_emulated.BOUND and hop_common.identity_bound of it.  These are bounds the suite already uses.  Two choices of E are
this file's own: a row's error is relative to the peak of the WHOLE oracle row (max(n0, ncols) columns), not of the ncols columns
that were written (ncols = 1 has no peak of its own), and the power of E is compared with the ORACLE's |W|^2, there being no W
of the same plan at that shape, within 2 TOL + 32 eps of the peak power: d|W|^2 <= 2 |W| d|W| <= 2 TOL peak^2 to first order,
plus the 32 eps that power_bound allows the square.

Straddling (switch_common.assert_straddling): after the call a pair counts only if its two rows still carry different labels;
at most one pair in ten may drop out, the rest number at least 4.  The families of switches that must occur are
switch_common.FAMILIES.

What a deliberately broken classifier fails first here (each tried once on a copy of the sources, none committed):
  poly_candidate   poly_degree_for with 100 x eps        test_values_at_every_switch_pair[2^15-fp64-morlet6-1e-12-white]:
                                                         poly/K256/d6 at 1.0e-11 of its peak
  gates            time_halo_factor with 1000 x tol.halo same case: ols/K256/half at 1.5e-10
                   profile_support with 1000 x tol.clip  same case: ols/K4096/half (a row that no longer vanishes at Nyquist) 4.5e-11
  classify_row     t1 = rd.nband >> 10                   ...[2^15-fp64-paul4-0-white]: narrow/K1024 with nband = 1024 + a few at 8.0e-8
                   need <= g.narrow_cap + 1              ...[2^15-fp64-morlet6-0-white] in assert_families (ols <-> narrow is gone);
                                                         with that assertion taken out ...[2^15-fp32-paul4-0-white]: narrow/K1024/t3
                                                         at 3.3e-3 (fp64 rows of the wider tile stay exact: only fp32 has no such tile)
  block_row        the k_lo alignment loop skipped       ...[2^15-fp64-morlet6-0-white]: ols/K256/half at 0.34
  ols_candidate    hh > cap + 64, halo > ols_hmax + 64   ...[2^15-fp64-paul4-1e-06-white] in assert_families only (ols <-> narrow_k2048
                                                         moves below narrow_k2048 <-> narrow); the values hold: the limit is tuning
                   two.logK <= ls - 2                    survives, as it may: the labels change for fp32 Paul at 3e-5 only (K = 1024
                                                         on blocks of two half-size tiles), the rows stay within 3e-5 -- K <= P / 8
                                                         keeps the stores in 128-byte segments, it is no capability of the kernel
  poly_candidate   best_deg <= POLY_MAX_DEGREE + 2       survives, as it must: no label of any probe grid of this file changes (all
                                                         sizes, mothers, precisions and targets compared).  The largest degree a
                                                         row takes is 12 of 24: K' <= poly_max_logk ends the form long before

fp64 Paul(4) at N = 2^18 and 1e-9 is the case that needs the second part of find_switches: a call over the whole range shows
three switches (two_pass/c16 <-> narrow_k2048/t6, t6 <-> t5, t5 <-> t4) and hides two_pass/full <-> c64 <-> c16 under rows that it
moves to the band-passed form; in the call of the pairs two_pass/c64 <-> c16 straddles with the other three (four pairs, none drops
out); two_pass/full <-> c64 does not hold in that call and is left out.
"""
import numpy as np
import pytest

import switch_common as sc
from hop_common import identity_bound
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND, FORMS_OPTS, numpy_adjoint, rel
from test_kernels_emulated import TOL
from test_power_emulated import EPS32, power_bound
from test_weighted_emulated import weighted_bound

MOTHERS = sc.MOTHERS
BENCH = sc.BENCH
value_cases, rows_cases, case_id = sc.value_cases, sc.rows_cases, sc.case_id


def bound_of(prec, target):
    return max(target, TOL[prec]) if target else TOL[prec]


def check_values(lib, logn, prec, kind, param, target, signal, most=None, with_signal=True):
    """A (and B with with_signal = False): the result, after its assertions"""
    N = 1 << logn
    r = sc.run_pairs(lib, N, N - sc.N0_OFF, prec, kind, param, sc.SIZES[logn], target, signal, with_signal=with_signal, most=most)
    print("%s%s: %d pairs, worst row: scale %.17g %s error %.3e (bound %.1e)" % (
        case_id((logn, prec, kind, param, target, signal)), "" if with_signal else "-rows", len(r.pairs), *r.worst(),
        bound_of(prec, target)))
    keep = sc.assert_straddling(r)
    sc.assert_families((logn, prec, sc.mother_id(kind, param), target, with_signal), sc.families_of(r, keep))
    for p in r.pairs:
        assert p[1] == np.nextafter(p[0], np.inf) and p[2] != p[3], p
    assert r.err.max() <= bound_of(prec, target), (r.worst(), bound_of(prec, target))
    return r


# ---- A ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", value_cases(15), ids=case_id)
def test_values_at_every_switch_pair(emu_library, case):
    check_values(emu_library, *case)


@pytest.mark.parametrize("case", value_cases(18), ids=case_id)
def test_values_at_every_switch_pair_of_the_production_gates(emu_library, case):
    check_values(emu_library, *case)


# ---- B ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rows_cases(), ids=case_id)
def test_spectrum_only_entry_point_at_its_own_switches(emu_library, case):
    """forward_fft + cwt_transform_rows: find_switches(with_signal = False)"""
    r = check_values(emu_library, *case, with_signal=False)
    assert not any(c.startswith("ols") for c in r.classes), r.classes


# ---- C ----------------------------------------------------------------------------------------------------------------------
def output_cases():
    return [(15, prec, kind, param, target) for prec in (64, 32) for kind, param in MOTHERS for target in (0.0, BENCH[prec])]


def check_power_and_weighted(lib, logn, prec, kind, param, target):
    N = 1 << logn
    r = sc.run_pairs(lib, N, N - sc.N0_OFF, prec, kind, param, sc.SIZES[logn], target, "white", extras=("power", "weighted"))
    sc.assert_straddling(r)
    perr = power_bound(r.P, r.W, prec)
    worst = weighted_bound(r.Gw, r.W, r.Q, sc.ALPHA, prec)
    print("2^%d-fp%d-%s-%g: power %.3e (row %s), weighted %.3e (bound %.1e)" % (
        logn, prec, sc.mother_id(kind, param), target, perr.max(), r.classes[int(perr.argmax())], worst, EPS32[prec]))


@pytest.mark.parametrize("case", output_cases(), ids=lambda c: case_id(c + ("white",)))
def test_power_and_weighted_outputs_at_the_pairs(emu_library, case):
    """cwt_transform_power against re^2 + im^2, cwt_transform_weighted (alpha = -0.75, Q with exact zeros and both signs) against
    alpha Q W, of the W of the same plan"""
    check_power_and_weighted(emu_library, *case)


# ---- D ----------------------------------------------------------------------------------------------------------------------
def adjoint_cases():
    return [(prec, kind, param, None) for prec in (64, 32) for kind, param in MOTHERS] + [(64, orc.MORLET, 6, 0)]


def check_adjoint(lib, prec, kind, param, adjoint_poly):
    N = 1 << 15
    r = sc.run_pairs(lib, N, N - sc.N0_OFF, prec, kind, param, FORMS_OPTS, 0.0, "white", extras=("adjoint",),
                     adjoint_poly=adjoint_poly)
    sc.assert_straddling(r)
    G = r.G.astype(np.complex128)
    ref = numpy_adjoint(G, r.sj, orc.Mother(kind, param), N)
    e = rel(r.xbar.astype(np.float64), ref)
    x = r.x.astype(np.float64)
    W = r.W.astype(np.complex128)
    lhs, rhs = float(np.real(np.vdot(G, W))), float(np.dot(x, r.xbar.astype(np.float64)))
    scale = max(np.linalg.norm(G) * np.linalg.norm(W), np.linalg.norm(x) * np.linalg.norm(r.xbar))
    print("fp%d-%s adjoint_poly %s: adjoint %.3e (bound %.1e), identity %.3e (bound %.1e)" % (
        prec, sc.mother_id(kind, param), adjoint_poly, e, BOUND[prec], abs(lhs - rhs) / scale, identity_bound(BOUND, prec)))
    assert e <= BOUND[prec], e
    assert abs(lhs - rhs) <= identity_bound(BOUND, prec) * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("prec,kind,param,adjoint_poly", adjoint_cases(),
                         ids=lambda v: None if v is None else str(v))
def test_adjoint_at_the_pairs(emu_library, prec, kind, param, adjoint_poly):
    """cwt_adjoint_rows with the pair scales after the forward of the same plan (the cached table) against the NumPy adjoint,
    and Re <G, A x> = <x, A^H G>; once with adjoint_poly = 0"""
    check_adjoint(emu_library, prec, kind, param, adjoint_poly)


# ---- E ----------------------------------------------------------------------------------------------------------------------
def shape_cases():
    return [(prec, kind, param, i) for prec in (64, 32) for kind, param in MOTHERS for i in range(len(sc.shapes(1 << 15)))]


def shape_id(c):
    return "fp%d-%s-n0_%d-ncols_%d-ld_%d" % ((c[0], sc.mother_id(c[1], c[2])) + sc.shapes(1 << 15)[c[3]])


def assert_forms(prec, kind, classes):
    forms = {c.split("/")[0] for c in classes}
    if kind != orc.PAUL:
        assert {"aols", "ols", "poly", "narrow"} <= forms, sorted(forms)
    elif prec == 64:
        assert {"two_pass", "narrow_k2048"} <= forms, sorted(forms)


def assert_padding(out, ncols, sentinel):
    pad = np.ascontiguousarray(out[:, ncols:])
    want = np.full(1, sentinel, dtype=out.dtype)
    assert np.all(pad.view(np.uint8).reshape(-1, want.nbytes) == want.view(np.uint8))          # the sentinel's bits


def check_shape(lib, prec, kind, param, i):
    N = 1 << 15
    n0, ncols, ldw = shape = sc.shapes(N)[i]
    out, classes, sj, ref, peak = sc.run_shape(lib, N, prec, kind, param, FORMS_OPTS, shape)
    assert_forms(prec, kind, classes)
    err = sc.row_error(out[:, :ncols], ref, peak)
    j = int(err.argmax())
    print("%s: %d rows, worst row: scale %.17g %s error %.3e" % (shape_id((prec, kind, param, i)), len(sj), sj[j], classes[j], err[j]))
    assert err.max() <= TOL[prec], (sj[j], classes[j], err[j])
    assert_padding(out, ncols, sc.SENTINEL * (1 + 1j))


@pytest.mark.parametrize("case", shape_cases(), ids=shape_id)
def test_ncols_other_than_n0_and_a_padded_leading_dimension(emu_library, case):
    """A 40-row grid over the whole range plus the switch pairs: the first ncols columns against the oracle's (transform length N,
    a signal of n0 samples), the padding columns keep the sentinel bit for bit; every form present"""
    check_shape(emu_library, *case)


def check_shape_power(lib, prec, kind, param, i):
    N = 1 << 15
    n0, ncols, ldw = shape = sc.shapes(N)[i]
    out, classes, sj, ref, peak = sc.run_shape(lib, N, prec, kind, param, FORMS_OPTS, shape, power=True)
    assert_forms(prec, kind, classes)
    pref = ref.real ** 2 + ref.imag ** 2
    err = np.abs(out[:, :ncols].astype(np.float64) - pref).max(axis=1) / peak ** 2
    j = int(err.argmax())
    print("%s power: worst row: scale %.17g %s error %.3e" % (shape_id((prec, kind, param, i)), sj[j], classes[j], err[j]))
    assert err.max() <= 2 * TOL[prec] + EPS32[prec], (sj[j], classes[j], err[j])
    assert_padding(out, ncols, sc.SENTINEL)


POWER_SHAPE_CASES = [(prec, kind, param, i) for prec in (64, 32) for kind, param in MOTHERS[:3] for i in (0, 3, 5)]


@pytest.mark.parametrize("case", POWER_SHAPE_CASES, ids=shape_id)
def test_power_with_ncols_other_than_n0(emu_library, case):
    check_shape_power(emu_library, *case)


# ---- F ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,param", MOTHERS, ids=[sc.mother_id(*m) for m in MOTHERS])
@pytest.mark.parametrize("prec", [64, 32])
def test_pairs_through_the_batch_call(emu_library, prec, kind, param):
    """cwt_transform_batch of 3 signals with x_ld = n0 + 5.  The batch counts toward the overlap-save threshold, so rows may take
    other forms than they do alone (printed); every (signal, row) within TOL of the oracle."""
    lib = emu_library
    real, cplx = sc.types(prec)
    es = np.dtype(real).itemsize
    N, nb = 1 << 15, 3
    n0 = N - sc.N0_OFF
    x_ld = n0 + 5
    m = orc.Mother(kind, param)
    X = np.zeros((nb, x_ld), dtype=real)
    for b in range(nb):
        X[b, :n0] = sc.signal("white", n0, prec, seed=30 + b)
    X[:, n0:] = 1e6                                          # (never read)
    plan = _hip.Plan(N, prec, max_rows=sc.MAX_ROWS, lib=lib, options=FORMS_OPTS)
    bufs = []
    try:
        pairs = sc.find_switches(plan, kind, param, n0, n0, True)
        sj = sc.pair_scales(pairs)
        rows = len(sj)
        for nbytes in (X.nbytes, nb * N * 2 * es, nb * rows * n0 * 2 * es):
            bufs.append(_hip.DeviceBuffer(nbytes, lib=lib))
        xd, xh, Wd = bufs
        xd.upload(plan, X)
        plan.transform_batch(xd.ptr, nb, x_ld, n0, kind, param, 1.0, sj, xh.ptr, Wd.ptr, n0, n0)
        classes = plan.row_classes()
        W = Wd.download(plan, (nb, rows, n0), cplx)
    finally:
        for b in bufs:
            b.free()
        plan.close()
    print("fp%d-%s batch: %d rows per signal, forms %s" % (prec, sc.mother_id(kind, param), rows, classes[:rows]))
    for b in range(nb):
        ref = orc.cwt_rows(X[b, :n0].astype(np.float64), 1.0, sj, m, N=N)[:, :n0]
        err = sc.row_error(W[b], ref, np.abs(ref).max(axis=1))
        assert err.max() <= TOL[prec], (b, sj[int(err.argmax())], classes[int(err.argmax())], err.max())
