"""The adjoint of the row transform (cwt_adjoint_rows, cwt_torch's backward) judged the way the forward is: every row ALONE,
against its own peak, on the CPU emulation of the HIP runtime (tests/emu).

A  every row of a grid alone in one batched call (signal b carries G in row b only: the batch loop and g_batch_ld), per row
   against  Re IDFT(conj F_b DFT(pad G_b))[:n0]  with the oracle's filter: relative 2-norm, and -- n0 = N -- the largest error
   of the spectrum of xbar_b relative to that spectrum's peak (the adjoint's "relative to the row's own peak");
B  single tones G_j[n] = e^{2 pi i k n / N} against the closed form  xbar[n] = Re(conj F_j[k] e^{2 pi i k n / N})  in longdouble:
   the peak, the two ends of the support and the bins next to them, the bins where the polynomial path wraps (kappa = +- K'/2),
   0, 1, N/2 - 1, N/2 and DOG's mirrored negative bins;
C  the polynomial rows in three or more chunks;  D  unsorted, repeated and subset scale grids;  E  the cached adjoint tables of
   a live plan (five grids over four slots, tolerance and adjoint_poly changed in between);  F  Paul through the transpose of
   the polynomial form;  G  cwt_torch's backward (real and non-contiguous upstream gradients, fp32 batches, two graphs alive on
   one engine, a tolerance changed between forward and backward, retain_graph).

Bounds, per row, none of them read off the kernels: at round-off test_adjoint_emulated.BOUND (1e-12 / 1e-5); with a tolerance
tol, max(10 tol, BOUND) -- the plan cuts every filter at 0.1 tol of the row's peak (plan_host.cpp `tolerances`), the polynomial
form and the overlap-save halo are truncated at the same 0.1 tol, so a row alone is within a few tenths of tol of its exact
adjoint in either metric; 10 tol is the bound test_polynomial_transpose_agrees_with_the_general_path already uses.  A tone's
error is relative to the peak of |F_j|; a tone outside the support returns at most the truncation, 10 tol peak.  The NumPy
reference itself (float64 FFTs against the longdouble closed form, N = 2^15) is good to ~1e-15 (test_reference_own_error).

Shapes: N = 2^15 with FORMS_OPTS (every row form at the smallest transform that has them all), 2^16 in complex64 (intervals of
R >= 128 samples); 17-row grids, so that a batch of "every row alone" costs 289 row transforms.  A runs both precisions at
n0 = N and N - 77, at round-off and at the bench target: the spectral metric exists at n0 = N only, so each precision meets its
round-off bound in it.

poly_moments_body's full-width tree (g = 256, logR = 14) needs N = 2^22 with K' = 256: half a minute here, fp64 Morlet only;
L > 64 (logR >= 15, N = 2^23) and the complex64 rows of both run in test_adjoint_forms_gpu.py only.

What a deliberately broken build fails first here (each tried once on a copy of the sources, none committed):
  k_poly_adj_accum  kap & (K/2 - 1); no sign for d & 2; the e^{i pi kappa / K'} shift one bit off   test_every_row_alone
  poly_moments_body rend without the n0 clip (n0 = N - 77); u without the - 1                       test_every_row_alone
  adjoint_impl      G + (first + i) ldg                                    test_unsorted_repeated_and_subset_scales
                    b nrows ldg for b g_batch_ld                  test_padded_rows_and_padded_batch_entries_of_the_input
                    a chunk's ks0 from the first chunk                     test_polynomial_rows_in_three_or_more_chunks
  plan_host.cpp     without t->adj_poly = -1      test_more_row_tables_than_slots, test_tolerance_changed_between_calls,
                                                  test_adjoint_poly_toggled_on_a_live_plan
  autograd.py       gW without .contiguous()             test_backward_with_non_contiguous_upstream_gradients
  k_adj_accum       band test >= to >: passes, as it must -- it admits the one bin k_lo + nband, which lies outside the
                    support (|F| below 0.1 tol of the peak, below 1e-17 at round-off), and adds that bin's CORRECT term
"""
import functools

import numpy as np
import pytest

from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND, FORMS_OPTS, adjoint, dense_operator, numpy_adjoint, random_g
from test_kernels_emulated import grid

BENCH_TOL = {64: 1e-9, 32: 3e-5}
ROWS = 17            # (the smallest grid on which every mother has every form it can have: assert_forms)
MOTHERS = [(orc.MORLET, 6), (orc.PAUL, 4), (orc.DOG, 2), (orc.DOG, 3)]


def bound_of(prec, tol):
    return max(10 * tol, BOUND[prec])


def types_of(prec):
    return (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)


def logn_of(prec):
    return 15 if prec == 64 else 16


def full_grid(N, m, rows):
    """grid() without dropping the rows the reference turns into NaN (Paul's largest scales: the rows that are narrow enough for
    the polynomial form); the oracle's intended-value filter defines them."""
    s0 = 2.0 / m.flambda()
    return s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))


@functools.lru_cache(maxsize=None)
def alone_case(kind, param, prec, n0_off, full=False, rows=ROWS):
    """(N, n0, mother, sj, g, ref): g (J x n0, in the precision's complex type) holds row j's input; ref[j] the float64 NumPy
    adjoint of row j alone.  Computed once per case and shared (read-only) by every test that needs it."""
    N = 1 << logn_of(prec)
    n0 = N - n0_off
    m = orc.Mother(kind, param)
    sj = full_grid(N, m, rows) if full else grid(N, 1.0, m, rows)
    g = random_g(np.random.default_rng(1000 * kind + param), len(sj), n0).astype(types_of(prec)[1])
    bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True)
    ref = np.real(np.fft.ifft(np.conj(bank) * np.fft.fft(g.astype(np.complex128), n=N, axis=1), axis=1))[:, :n0]
    for a in (sj, g, ref):
        a.setflags(write=False)
    return N, n0, m, sj, g, ref


def alone(g, order=None):
    """G (J x J x n0): signal b = row order[b] of g in row b, zeros elsewhere."""
    order = np.arange(g.shape[0]) if order is None else np.asarray(order)
    G = np.zeros((order.size, order.size, g.shape[1]), dtype=g.dtype)
    for b, j in enumerate(order):
        G[b, b] = g[j]
    return G


def row_errors_of(xbar, ref, spectral):
    """Per row: relative 2-norm, and (spectral) max_k |DFT(xbar - ref)[k]| / max_k |DFT(ref)[k]|."""
    d = xbar.astype(np.float64) - ref
    e2 = np.linalg.norm(d, axis=1) / np.linalg.norm(ref, axis=1)
    if not spectral:
        return e2, np.zeros_like(e2)
    return e2, np.abs(np.fft.fft(d, axis=1)).max(axis=1) / np.abs(np.fft.fft(ref, axis=1)).max(axis=1)


def assert_rows(xbar, ref, classes, bound, spectral):
    e2, es = row_errors_of(xbar, ref, spectral)
    print("per-row rel-2 / spectral:", " ".join(f"{c}:{a:.1e}/{b:.1e}" for c, a, b in zip(classes, e2, es)))
    assert e2.max() <= bound, (int(e2.argmax()), classes[e2.argmax()], e2.max())
    assert es.max() <= bound, (int(es.argmax()), classes[es.argmax()], es.max())


def poly_of(classes):
    """[(row, K', degree)] of the polynomial rows, read from the class strings."""
    return [(j, int(c.split("/")[1][1:]), int(c.split("/")[2][1:])) for j, c in enumerate(classes) if c.startswith("poly")]


def assert_forms(classes, kind, prec, full=False):
    """The table holds what the case is about.  Mother-specific exceptions, as test_every_row_form_against_a_numpy_adjoint: on the
    grid without the reference's NaN rows Paul has no polynomial row (the rows narrow enough are the dropped ones; F runs them
    on the full grid); fp64 Paul takes the band-passed form only at a looser target and has no overlap-save row at round-off
    (complex64 Paul has both); complex64 at 2^16 needs no narrow / two-pass row where overlap-save takes every wide row."""
    kinds = {c.split("/")[0] for c in classes}
    if kind != orc.PAUL or full:
        poly = poly_of(classes)
        assert len({k for _, k, _ in poly}) >= 2 and len({d for _, _, d in poly}) >= 2, classes
    if kind != orc.PAUL:
        assert "ols" in kinds and "aols" in kinds, classes
    if prec == 64:
        assert {"narrow", "two_pass", "narrow_k2048"} & kinds, classes


# ---- the reference ---------------------------------------------------------------------------------------------------------

def tone_reference(F, k, N):
    """Re(conj F e^{2 pi i k n / N}), n = 0 ... N-1, in longdouble (no FFT: the angle is reduced exactly in integers)."""
    ang = 8 * np.arctan(np.longdouble(1)) * np.asarray((np.arange(N, dtype=np.int64) * int(k)) % N, dtype=np.longdouble) / np.longdouble(N)
    Fr, Fi = np.longdouble(np.real(F)), np.longdouble(np.imag(F))
    return Fr * np.cos(ang) + Fi * np.sin(ang)


def test_tone_closed_form_is_the_dense_operators_adjoint():
    """Sign and normalisation of B's closed form (the comment above k_adj_accum: acc[k] = F[k]/N conj(DFT(G)[k]), xbar = Re DFT(acc)),
    once, against Re(A^H G) of the dense operator at N = 256: positive and negative bins, a real and an imaginary filter."""
    N = 256
    for kind, param, j, sign in ((orc.MORLET, 6, 3, 1), (orc.DOG, 3, 4, -1), (orc.DOG, 3, 4, 1), (orc.PAUL, 4, 2, 1)):
        m = orc.Mother(kind, param)
        sj = grid(N, 1.0, m, 8)
        F = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True)
        k = sign * (int(np.abs(F[j, :N // 2]).argmax()) + 1)       # next to the peak: not a symmetric point of the filter
        G = np.zeros((len(sj), N), dtype=np.complex128)
        G[j] = np.exp(2j * np.pi * k * np.arange(N) / N)
        ref = np.real(dense_operator(N, N, sj, m).conj().T @ G.reshape(-1))
        got = tone_reference(F[j, k % N], k, N).astype(np.float64)
        assert np.abs(F[j, k % N]) > 1e-3 and np.abs(got - ref).max() <= 1e-13 * np.abs(F[j]).max(), (kind, k)


def test_reference_own_error():
    """The float64 FFT reference of A against the longdouble closed form on a tone, and against itself in longdouble arithmetic
    of the same sum at N = 2^15: ~1e-16 log2 N, three orders below the fp64 bound."""
    N = 1 << 15
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, 1.0, m, ROWS)[8:9]
    F = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True)[0]
    k = int(np.abs(F).argmax())
    G = np.exp(2j * np.pi * ((k * np.arange(N)) % N) / N)[None, :]
    err = np.abs(numpy_adjoint(G, sj, m, N) - tone_reference(F[k], k, N)).max() / np.abs(F).max()
    print("reference, float64 FFTs against the longdouble closed form:", err)
    assert err <= 1e-14


# ---- A: every row alone ------------------------------------------------------------------------------------------------------

def run_alone(lib, kind, param, prec, n0_off, tol, opts=None, full=False, order=None, plan=None):
    N, n0, m, sj, g, ref = alone_case(kind, param, prec, n0_off, full)
    order = np.arange(len(sj)) if order is None else np.asarray(order)
    xbar, _, classes = adjoint(lib, N, prec, kind, param, sj[order], alone(g, order), dict(FORMS_OPTS, **(opts or {})), tol=tol,
                               plan=plan)
    return xbar, ref[order], classes


@pytest.mark.parametrize("prec,n0_off,target", [(64, 0, "roundoff"), (64, 77, "roundoff"), (64, 0, "bench"), (64, 77, "bench"),
                                                (32, 0, "roundoff"), (32, 77, "roundoff"), (32, 0, "bench"), (32, 77, "bench")])
@pytest.mark.parametrize("kind,param", MOTHERS)
def test_every_row_alone(emu_library, kind, param, prec, n0_off, target):
    """A.  One call, nbatch = J; both metrics per row (the spectral one at n0 = N).  DOG 3: an imaginary filter."""
    tol = BENCH_TOL[prec] if target == "bench" else 0.0
    xbar, ref, classes = run_alone(emu_library, kind, param, prec, n0_off, tol)
    assert_forms(classes, kind, prec)
    assert_rows(xbar, ref, classes, bound_of(prec, tol), n0_off == 0)


def run_long(lib, logn, kind, param, prec):
    """The three largest scales of a long series with K' held at 256 (poly_max_logk = 8), each alone in a batch of three, with
    adjoint_poly = 1 and 0: intervals of R = N / 256 samples, so k_poly_moments' tree is g = R / max(64, R / 256) wide -- the
    full 256 lanes from N = 2^22 -- and a thread sums L = R / 256 > 64 samples from N = 2^23.  Returns the per-row errors (relative
    2-norm, spectral) of both paths and the classes."""
    N = 1 << logn
    m = orc.Mother(kind, param)
    sj = grid(N, 1.0, m, 64)[-3:]
    g = random_g(np.random.default_rng(logn), 3, N).astype(types_of(prec)[1])
    bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True)
    ref = np.real(np.fft.ifft(np.conj(bank) * np.fft.fft(g.astype(np.complex128), axis=1), axis=1))
    out, seen = [], []
    for flag in (1, 0):
        xbar, _, classes = adjoint(lib, N, prec, kind, param, sj, alone(g), {"poly_max_logk": 8, "adjoint_poly": flag})
        out.append(row_errors_of(xbar, ref, True))
        seen.append(classes)
    assert seen[0] == seen[1], seen          # (the option changes the adjoint's path, not the table: the classes are those of both)
    return out, seen[0]


@pytest.mark.slow
def test_long_series_full_width_tree(emu_library):
    """poly_moments_body with logR = 14: L = 64 and the tree over all 256 lanes of the workgroup (every other case here has
    g <= 64), fp64 Morlet at N = 2^22, through both paths."""
    (poly, general), classes = run_long(emu_library, 22, orc.MORLET, 6, 64)
    assert all(c.startswith("poly/K256/") for c in classes), classes
    for errs in (poly, general):
        assert max(errs[0].max(), errs[1].max()) <= BOUND[64], (classes, errs)


# ---- B: single tones -----------------------------------------------------------------------------------------------------------

def support_eps(prec, tol):
    """plan_host.cpp `tolerances`: bins below this fraction of the row's peak are treated as zero."""
    t = tol if tol > 0 else (1e-16 if prec == 64 else 1e-8)
    return max(0.1 * t, 1e-18 if prec == 64 else 1e-9)


def tone_bins(F, N, eps, kprime, two_sided):
    """Signed bins of B for one row: the peak; the first and last bin above the support threshold, one and two bins beyond each
    and one inside; 0, 1, N/2 - 1, -N/2; with K' (polynomial rows) the carrier -- the band's centre, and the peak, which is where
    the classifier moves it for a lopsided filter -- +- K'/2 and +- (K'/2 - 1) inside the band; for DOG the mirror of all of them."""
    mag = np.abs(np.fft.fftshift(F))                           # signed bins -N/2 ... N/2 - 1
    half = N // 2
    pos = mag[half:]
    peak = int(pos.argmax())
    above = np.nonzero(pos > eps * pos.max())[0]
    lo, hi = int(above[0]), int(above[-1])
    bins = {peak, 0, 1, half - 1, -half}
    for e, s in ((lo, -1), (hi, 1)):
        bins.update(e + s * i for i in (-1, 0, 1, 2))
    if kprime:
        for kc in {(lo + hi + 1) // 2, peak}:
            for dk in (0, kprime // 2, kprime // 2 - 1):
                bins.update(k for k in (kc + dk, kc - dk) if lo <= k <= hi)
    if two_sided:
        bins.update([-k for k in bins])
    return sorted(k for k in bins if -half <= k < half), (lo, hi)


def run_tones(lib, kind, param, prec, tol, full=False, opts=None):
    """Every polynomial row and one row of every other class of the case's grid, each as a call of its own row (nrows = 1: a
    tone's batch entry then costs one row, not J), one batch entry per tone.  The one-row call classifies the row as the grid's
    call does (asserted)."""
    N, _, m, sj, _, _ = alone_case(kind, param, prec, 0, full)
    cplx = types_of(prec)[1]
    opts = dict(FORMS_OPTS, **(opts or {}))
    plan = _hip.Plan(N, prec, max_rows=len(sj), lib=lib, options=opts)
    if tol:
        plan.set_tolerance(tol)
    classes = plan.classify(kind, param, 1.0, sj, N, True)
    seen, chosen = set(), []
    for j, c in enumerate(classes):
        if c.startswith("poly") or c.split("/")[0] not in seen:
            chosen.append(j)
        seen.add(c.split("/")[0])
    bank = orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True)
    n = np.arange(N, dtype=np.int64)
    worst = []
    for j in chosen:
        kp = int(classes[j].split("/")[1][1:]) if classes[j].startswith("poly") else 0
        bins, (lo, hi) = tone_bins(bank[j], N, support_eps(prec, tol), kp, kind == orc.DOG)
        G = np.exp(2j * np.pi * ((np.asarray(bins)[:, None] * n[None, :]) % N) / N).astype(cplx)[:, None, :]
        xbar, _, one = adjoint(lib, N, prec, kind, param, sj[j:j + 1], G, plan=plan)
        assert one == [classes[j]], (one, classes[j])
        peak = np.abs(bank[j]).max()
        for b, k in enumerate(bins):
            ref = tone_reference(bank[j, k % N], k, N)
            err = float(np.abs(xbar[b] - ref).max() / peak)
            worst.append((err, j, classes[j], k, (lo, hi)))
            assert err <= bound_of(prec, tol), worst[-1]
            if np.abs(bank[j, k % N]) <= support_eps(prec, tol) * peak:      # outside the support: what the truncation allows
                assert float(np.abs(xbar[b]).max()) <= bound_of(prec, tol) * peak, (worst[-1], float(np.abs(xbar[b]).max()))
    plan.close()
    print("worst tone (error / peak, row, class, bin, support):", max(worst))
    return classes, chosen


@pytest.mark.parametrize("kind,param,prec,target", [
    (orc.MORLET, 6, 64, "roundoff"), (orc.MORLET, 6, 64, "bench"), (orc.DOG, 2, 64, "bench"), (orc.DOG, 3, 32, "bench")])
def test_single_tones_against_the_closed_form(emu_library, kind, param, prec, target):
    """B.  An off-by-one at k_lo or k_lo + nband - 1, a wrong wrap of kappa at +- K'/2, a wrong i^d or rotation changes one bin
    of one row: that bin alone is the input here."""
    tol = BENCH_TOL[prec] if target == "bench" else 0.0
    classes, chosen = run_tones(emu_library, kind, param, prec, tol)
    assert len({classes[j].split("/")[0] for j in chosen}) >= 3, classes


# ---- C: polynomial chunks ------------------------------------------------------------------------------------------------------

def chunk_case(kind, param, prec):
    """The polynomial rows with K' >= 512 of a dense grid at N = 2^16: over 2 MiB of coefficient planes (the grids of A hold
    under 1 MiB, and 1 MiB is the smallest chunk limit there is); rows alone = the first, the last and every eighth row."""
    N = 1 << 16
    m = orc.Mother(kind, param)
    return N, m, grid(N, 1.0, m, {64: 220, 32: 680}[prec])


@pytest.mark.parametrize("kind,param,prec", [(orc.MORLET, 6, 64), (orc.DOG, 2, 32), (orc.MORLET, 6, 32)])
def test_polynomial_rows_in_three_or_more_chunks(emu_library, kind, param, prec):
    """C.  poly_chunk_mb = 1 against one chunk: the chunk count from the plan's own launch counts (profile: every chunk adds one
    k_poly_moments and one k_poly_adj_accum launch to the class "adjoint"); rows alone within the per-row bounds; the whole sum
    within round-off of the one-chunk run.  The bits need not be those of the one-chunk run -- a bin that rows of two chunks
    share is added to acc in two steps instead of one -- but a row alone is added once either way: its bits are equal.
    Morlet in complex64 as well: at 1e-9 every Morlet band starts at the clamp next to bin 0 and DOG's widest bands (the first
    chunk: largest K' first) start lowest, so only here does a later chunk's band union start BELOW the first chunk's."""
    N, m, sj = chunk_case(kind, param, prec)
    tol = BENCH_TOL[prec]
    cplx = types_of(prec)[1]
    probe = _hip.Plan(N, prec, max_rows=len(sj), lib=emu_library, options=FORMS_OPTS)
    probe.set_tolerance(tol)
    sj = sj[[j for j, k, _ in poly_of(probe.classify(kind, param, 1.0, sj, N, True)) if k >= 512]]
    probe.close()
    J = len(sj)
    rng = np.random.default_rng(8)
    g = random_g(rng, J, N).astype(cplx)
    picks = sorted(set(range(0, J, 8)) | {J - 1})
    G = np.zeros((len(picks) + 1, J, N), dtype=cplx)
    for b, j in enumerate(picks):
        G[b, j] = g[j]
    G[-1] = g
    out, counts = {}, {}
    for mb in (0, 1):
        plan = _hip.Plan(N, prec, max_rows=J, lib=emu_library, options=dict(FORMS_OPTS, poly_chunk_mb=mb, profile=1))
        plan.set_tolerance(tol)
        out[mb], _, classes = adjoint(emu_library, N, prec, kind, param, sj, G, plan=plan)
        plan.sync()
        counts[mb] = plan.timings()["adjoint"][1]
        plan.close()
    assert all(c.startswith("poly") for c in classes), classes
    chunks = 1 + (counts[1] - counts[0]) / (2 * G.shape[0])
    assert chunks >= 3 and chunks == int(chunks), (counts, chunks)
    bank = orc.filter_bank(sj[picks], orc.angular_freqs(N, 1.0), N, m, True)
    ref = np.real(np.fft.ifft(np.conj(bank) * np.fft.fft(g[picks].astype(np.complex128), axis=1), axis=1))
    assert_rows(out[1][:-1], ref, [classes[j] for j in picks], bound_of(prec, tol), True)
    np.testing.assert_array_equal(out[1][:-1], out[0][:-1])
    whole = np.linalg.norm(out[1][-1] - out[0][-1]) / np.linalg.norm(out[0][-1])
    assert whole <= BOUND[prec], whole


# ---- D: row order ----------------------------------------------------------------------------------------------------------------

def shuffled_order(classes, seed=4):
    """The rows permuted, a polynomial and a general row adjacent in every second position, two scales repeated."""
    rng = np.random.default_rng(seed)
    poly = [j for j, c in enumerate(classes) if c.startswith("poly")]
    gen = [j for j, c in enumerate(classes) if not c.startswith("poly")]
    poly, gen = list(rng.permutation(poly)), list(rng.permutation(gen))
    order = []
    while poly or gen:
        if poly:
            order.append(poly.pop())
        if gen:
            order.append(gen.pop())
    order[3:3] = [order[-1]]                                   # a general row twice, apart
    return np.array(order + [order[0]])                        # a polynomial row twice, first and last


@pytest.mark.parametrize("kind,param,prec,target", [(orc.MORLET, 6, 64, "bench"), (orc.DOG, 3, 32, "roundoff")])
def test_unsorted_repeated_and_subset_scales(emu_library, kind, param, prec, target):
    """D.  Table order differs from out_row order and the polynomial / general split interleaves: xbar of every row alone has
    the bits of the sorted run's row of that scale (a row's form and arithmetic do not depend on its neighbours, and the rows
    that carry zeros add exact zeros); so has a nine-row subset."""
    tol = BENCH_TOL[prec] if target == "bench" else 0.0
    sorted_x, _, classes = run_alone(emu_library, kind, param, prec, 77, tol)
    order = shuffled_order(classes)
    assert len(order) == len(classes) + 2
    x, ref, c2 = run_alone(emu_library, kind, param, prec, 77, tol, order=order)
    assert c2 == [classes[j] for j in order]
    assert sum(a.startswith("poly") != b.startswith("poly") for a, b in zip(c2[::2], c2[1::2])) >= len(c2) // 2 - 4, c2
    assert_rows(x, ref, c2, bound_of(prec, tol), False)
    np.testing.assert_array_equal(x, sorted_x[order])
    nine = order[[1, 2, 5, 6, 9, 10, 13, 14, 16]]
    x9, _, c9 = run_alone(emu_library, kind, param, prec, 77, tol, order=nine)
    assert any(c.startswith("poly") for c in c9) and not all(c.startswith("poly") for c in c9), c9
    np.testing.assert_array_equal(x9, sorted_x[nine])


# ---- E: cached state ---------------------------------------------------------------------------------------------------------

class Live:
    """One plan with max_rows fixed, and the forward / adjoint calls a training loop makes on it."""
    N, prec, kind, param = 1 << 15, 64, orc.MORLET, 6
    n0 = N - 77

    def __init__(self, lib, **opts):
        self.lib = lib
        self.plan = _hip.Plan(self.N, self.prec, max_rows=ROWS, lib=lib, options=dict(FORMS_OPTS, **opts))

    def forward(self, sj, ldw=None):
        ldw = ldw or self.n0
        xd, Wd = _hip.DeviceBuffer(self.n0 * 8, lib=self.lib), _hip.DeviceBuffer(len(sj) * ldw * 16, lib=self.lib)
        xd.upload(self.plan, np.random.default_rng(2).standard_normal(self.n0))
        self.plan.transform(xd.ptr, self.n0, self.kind, self.param, 1.0, sj, None, Wd.ptr, ldw, self.n0)
        W = Wd.download(self.plan, (len(sj), ldw), np.complex128)[:, :self.n0]
        xd.free(); Wd.free()
        return W

    def adjoint(self, sj):
        G = random_g(np.random.default_rng(len(sj)), 1, len(sj), self.n0)
        return adjoint(self.lib, self.N, self.prec, self.kind, self.param, sj, G, plan=self.plan)[0]

    def close(self):
        self.plan.close()


def three_grids():
    return five_grids()[:3]


def five_grids():
    """Five values of dj: one row table more than the plan's cache has slots (four)."""
    m = orc.Mother(Live.kind, Live.param)
    return [grid(Live.N, 1.0, m, rows) for rows in (ROWS, ROWS - 3, ROWS - 5, ROWS - 1, ROWS - 4)]


def fresh(lib, sj, tol=0.0, **opts):
    live = Live(lib, **opts)
    if tol:
        live.plan.set_tolerance(tol)
    out = live.adjoint(sj)                                    # (an adjoint with no forward before it)
    live.close()
    return out


def test_more_row_tables_than_slots(emu_library):
    """E.  The cache holds four row tables (plan.hpp), so five grids: forwards of g1 ... g5 (g5 evicts g1), then adjoints of g1, g3,
    g5, g2, g4, g1 -- the later ones rebuild their table in a slot whose adjoint rows were uploaded for ANOTHER grid, stale until
    upload_row_table says so (adj_poly = -1) -- then forwards that evict again and the adjoints once more.  Every result has the
    bits of the same adjoint on a fresh plan that never ran a forward."""
    grids = five_grids()
    assert len({len(sj) for sj in grids}) == 5
    want = [fresh(emu_library, sj) for sj in grids]
    live = Live(emu_library)
    for sj in grids:
        live.forward(sj)
    for i in (0, 2, 4, 1, 3, 0):
        np.testing.assert_array_equal(live.adjoint(grids[i]), want[i], err_msg=f"grid {i}")
    for i in (1, 2):
        live.forward(grids[i])
    for i in (4, 3, 2, 1, 0):
        np.testing.assert_array_equal(live.adjoint(grids[i]), want[i], err_msg=f"grid {i} after forwards evicted its slot")
    live.close()


ORDER = (0, 2, 4, 1, 3, 0)      # adjoints after the forwards of g1 ... g5: g1's table was evicted by g5's, every later one evicts again


def test_tolerance_changed_between_calls(emu_library):
    """E.  The sequence of test_more_row_tables_than_slots with set_tolerance 0 -> 1e-9 -> 0 -> ... before every adjoint:
    the tolerance is part of the table's key, so five grids at two tolerances are ten tables over four slots, and each adjoint
    has the bits of a fresh plan at that grid and tolerance (and the two tolerances really differ)."""
    grids = five_grids()
    want = {(i, tol): fresh(emu_library, grids[i], tol) for i in set(ORDER) for tol in (0.0, 1e-9)}
    assert all(not np.array_equal(want[i, 0.0], want[i, 1e-9]) for i in set(ORDER))
    live = Live(emu_library)
    for sj in grids:
        live.forward(sj)
    for n, i in enumerate(ORDER + ORDER[1:4]):
        tol = (0.0, 1e-9)[n % 2]
        live.plan.set_tolerance(tol)
        if n % 3 == 2:
            live.forward(grids[i])                            # (and a forward at the new tolerance before some of them)
        np.testing.assert_array_equal(live.adjoint(grids[i]), want[i, tol], err_msg=f"call {n}: grid {i} at {tol}")
    live.close()


def test_adjoint_poly_toggled_on_a_live_plan(emu_library):
    """E.  The same sequence with adjoint_poly 1 -> 0 -> 1 on every table in turn: upload_adjoint_rows must notice the option
    (adj_poly of the slot) and a slot's new tenant (adj_poly = -1), or the general path would skip the polynomial rows that
    nobody then adds, or add another grid's rows -- plausible-looking wrong gradients.  The second result is that of a fresh
    adjoint_poly = 0 plan, the third has the bits of the first."""
    grids = five_grids()
    want = {(i, flag): fresh(emu_library, grids[i], adjoint_poly=flag) for i in set(ORDER) for flag in (1, 0)}
    assert all(not np.array_equal(want[i, 0], want[i, 1]) for i in set(ORDER))
    live = Live(emu_library)
    for sj in grids:
        live.forward(sj)
    for i in ORDER:
        got = []
        for flag in (1, 0, 1):
            live.plan.set_option("adjoint_poly", flag)
            got.append(live.adjoint(grids[i]))
        np.testing.assert_array_equal(got[0], want[i, 1], err_msg=f"grid {i}")
        np.testing.assert_array_equal(got[1], want[i, 0], err_msg=f"grid {i}")
        np.testing.assert_array_equal(got[2], got[0], err_msg=f"grid {i}")
    live.close()


def test_forward_with_a_padded_leading_dimension_then_the_adjoint(emu_library):
    """E.  A forward whose ldw != ncols shares its table with the adjoint (ldw is no part of the key): same W, same xbar."""
    sj = three_grids()[1]
    want = fresh(emu_library, sj)
    live = Live(emu_library)
    W = live.forward(sj)
    Wp = live.forward(sj, ldw=Live.n0 + 13)
    np.testing.assert_array_equal(Wp, W)
    np.testing.assert_array_equal(live.adjoint(sj), want)
    live.close()


def test_padded_rows_and_padded_batch_entries_of_the_input(emu_library):
    """ldg > ncols and g_batch_ld > nrows ldg, the padding NaN, xbar_ld > ncols: the bits of the compact call, and the gaps of
    xbar untouched."""
    sj = three_grids()[2]
    n0, rows, nb = Live.n0, len(three_grids()[2]), 3
    ldg, gap, xld = n0 + 5, 11, n0 + 3
    G = random_g(np.random.default_rng(12), nb, rows, n0)
    live = Live(emu_library)
    want = adjoint(emu_library, Live.N, 64, Live.kind, Live.param, sj, G, plan=live.plan)[0]
    wide = np.full((nb, rows * ldg + gap), np.nan + 1j * np.nan)
    wide[:, :rows * ldg].reshape(nb, rows, ldg)[:, :, :n0] = G
    Gd = _hip.DeviceBuffer(wide.nbytes, lib=emu_library)
    xb = _hip.DeviceBuffer(nb * xld * 8, lib=emu_library)
    Gd.upload(live.plan, wide)
    xb.upload(live.plan, np.full(nb * xld, 7.25))
    live.plan.adjoint_rows(Gd.ptr, nb, rows * ldg + gap, ldg, n0, Live.kind, Live.param, 1.0, sj, xb.ptr, xld)
    got = xb.download(live.plan, (nb, xld), np.float64)
    Gd.free(); xb.free()
    live.close()
    np.testing.assert_array_equal(got[:, :n0], want)
    assert np.all(got[:, n0:] == 7.25)


def test_row_counts_the_plan_cannot_hold_are_refused_before_any_launch(emu_library):
    """E.  The row table's key carries nrows, so a cached table can never describe another row count (upload_adjoint_rows' own
    check is a second line of defence that the ABI cannot reach); what a caller can get wrong is a row count beyond max_rows, or
    a batch stride that lets signals overlap: CWT_EINVAL, and xbar is not touched."""
    sj = three_grids()[0]
    live = Live(emu_library)
    live.forward(sj)
    n0 = Live.n0
    Gd = _hip.DeviceBuffer((ROWS + 1) * n0 * 16 * 2, lib=emu_library)
    xb = _hip.DeviceBuffer(2 * n0 * 8, lib=emu_library)
    mark = np.full(2 * n0, 7.25)
    xb.upload(live.plan, mark)
    more = np.concatenate([sj, sj[:1]])[:ROWS + 1]
    with pytest.raises(_hip.HipError, match="max_rows") as e:
        live.plan.adjoint_rows(Gd.ptr, 1, len(more) * n0, n0, n0, Live.kind, Live.param, 1.0, more, xb.ptr, n0)
    assert e.value.code == -1                                  # CWT_EINVAL
    with pytest.raises(_hip.HipError, match="g_batch_ld") as e:
        live.plan.adjoint_rows(Gd.ptr, 2, len(sj) * n0 - 1, n0, n0, Live.kind, Live.param, 1.0, sj, xb.ptr, n0)
    assert e.value.code == -1
    np.testing.assert_array_equal(xb.download(live.plan, (2 * n0,), np.float64), mark)
    np.testing.assert_array_equal(live.adjoint(sj), fresh(emu_library, sj))      # and the plan is as good as new
    Gd.free(); xb.free()
    live.close()


# ---- F: Paul through the transpose of the polynomial form -------------------------------------------------------------------------

@pytest.mark.parametrize("prec,target", [(64, "roundoff"), (64, "bench"), (32, "bench")])
def test_paul_rows_alone_through_the_polynomial_form(emu_library, prec, target):
    """F.  Paul 4 has polynomial rows as soon as the grid keeps the scales the reference turns into NaN (the largest ones: the
    only ones narrow enough, B <= N / 64) -- N = 2^15 with FORMS_OPTS is enough, no looser target or other option is needed.
    Paul's band starts at bin 1 by construction (row_support), so no polynomial row of Paul reaches below bin 0: the bands that
    do, with k = ks & (N - 1), are DOG's, in A and B above.  The carrier is not reported by the plan; asserted are, from the
    oracle's filter, the condition under which the classifier looks for one off the centre: a peak further than 1/16 of the band
    from the band's centre (Paul: at ~9 % of the band) -- and its effect: the search keeps the centre unless another carrier has a
    strictly lower degree at some K' (poly_candidate), so a row whose K' or degree differs from the same row's under
    poly_carrier = 0 (the centre, always) runs with kc_off != nband / 2."""
    tol = BENCH_TOL[prec] if target == "bench" else 0.0
    xbar, ref, classes = run_alone(emu_library, orc.PAUL, 4, prec, 0, tol, full=True)
    assert_forms(classes, orc.PAUL, prec, full=True)
    N, _, m, sj, _, _ = alone_case(orc.PAUL, 4, prec, 0, True)
    centred = _hip.Plan(N, prec, max_rows=len(sj), lib=emu_library, options=dict(FORMS_OPTS, poly_carrier=0))
    if tol:
        centred.set_tolerance(tol)
    at_centre = centred.classify(orc.PAUL, 4, 1.0, sj, N, True)
    centred.close()
    moved = [(c, at_centre[j]) for j, c in enumerate(classes) if c.startswith("poly") and c != at_centre[j]]
    print("carrier off the centre (class, class with poly_carrier = 0):", moved)
    assert len(moved) >= 2, (classes, at_centre)
    bank = np.abs(orc.filter_bank(sj, orc.angular_freqs(N, 1.0), N, m, True))
    lopsided = 0
    for j, _, _ in poly_of(classes):
        above = np.nonzero(bank[j, :N // 2] > support_eps(prec, tol) * bank[j].max())[0]
        lo, hi = int(above[0]), int(above[-1])
        assert lo >= 1
        lopsided += hi - lo > 16 and abs(2 * int(bank[j].argmax()) - (lo + hi)) * 8 > hi - lo + 1
    assert lopsided >= 3, classes
    assert_rows(xbar, ref, classes, bound_of(prec, tol), True)


@pytest.mark.parametrize("prec,target", [(64, "bench")])
def test_paul_single_tones_through_the_polynomial_form(emu_library, prec, target):
    tol = BENCH_TOL[prec] if target == "bench" else 0.0
    classes, chosen = run_tones(emu_library, orc.PAUL, 4, prec, tol, full=True)
    assert sum(classes[j].startswith("poly") for j in chosen) >= 4, classes


# ---- G: cwt_torch ----------------------------------------------------------------------------------------------------------------

torch = None


@pytest.fixture()
def torch_emulated(emulated):
    """The shim on the emulated library, and torch (these tests alone need it: A to F run without)."""
    global torch
    torch = pytest.importorskip("torch")
    return emulated


def torch_case(n0=100, dj=1 / 4, wavelet="morlet", dtype=None, batch=None, seed=0):
    import pycwt_amd
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((n0,) if batch is None else (batch, n0), dtype=dtype or torch.float64, generator=gen, requires_grad=True)
    W, sj, _, _ = pycwt_amd.cwt_torch(x, 1.0, dj, wavelet=wavelet)
    return x, W, sj


@functools.lru_cache(maxsize=None)
def dense_of(n0, N, dj, wavelet):
    m = orc.mother_from_name(wavelet)
    sj, _ = orc.scale_grid(n0, 1.0, dj, -1, -1, m)
    return dense_operator(n0, N, sj, m)


def expected_grad(gW, n0, N, dj, wavelet="morlet"):
    """Re(A^H gW) of the dense operator, per signal."""
    A = dense_of(n0, N, dj, wavelet)
    g = np.asarray(gW, dtype=np.complex128).reshape(-1, A.shape[0])
    return np.real(g @ A.conj())


def close_to(a, b, bound):
    return np.linalg.norm(np.ravel(a - b)) <= bound * np.linalg.norm(np.ravel(b))


def test_backward_with_a_real_upstream_gradient(torch_emulated):
    """G.  loss = sum Re W: the gradient autograd hands to the backward is 1 + 0i; and a float64 gradient given outright
    (backward's gW.to(cplx_t))."""
    x, W, sj = torch_case()
    W.real.sum().backward()
    want = expected_grad(np.ones(W.shape), 100, 128, 1 / 4)[0]
    assert close_to(x.grad.numpy(), want, 1e-12)
    x2, W2, _ = torch_case()
    Wr = torch.view_as_real(W2)[..., 0]
    gen = torch.Generator().manual_seed(5)
    gr = torch.randn(Wr.shape, dtype=torch.float64, generator=gen)
    (g2,) = torch.autograd.grad(Wr, x2, grad_outputs=gr)
    assert close_to(g2.numpy(), expected_grad(gr.numpy(), 100, 128, 1 / 4)[0], 1e-12)


def test_backward_with_non_contiguous_upstream_gradients(torch_emulated):
    """G.  Losses over W[..., ::2] and over W.transpose(-1, -2): whatever strides autograd gives gW, the kernels read rows of n0
    consecutive values."""
    w = torch.randn(100, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    x, W, _ = torch_case()
    (W[..., ::2] * w[::2]).abs().pow(2).sum().backward()
    g = np.zeros(W.shape, dtype=np.complex128)
    g[:, ::2] = 2 * (W.detach().numpy() * w.numpy() ** 2)[:, ::2]
    assert close_to(x.grad.numpy(), expected_grad(g, 100, 128, 1 / 4)[0], 1e-12)
    x, W, _ = torch_case(batch=2)
    Wt = W.transpose(-1, -2)
    gt = torch.randn(Wt.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).to(torch.complex128) * (1 + 2j)
    assert not gt.transpose(-1, -2).is_contiguous()
    (gx,) = torch.autograd.grad(Wt, x, grad_outputs=gt)
    assert close_to(gx.numpy(), expected_grad(gt.transpose(-1, -2).numpy(), 100, 128, 1 / 4), 1e-12)


def test_fp32_batch_against_the_dense_operator(torch_emulated):
    """G.  A (3, n0) float32 batch: nb = g.shape[0], g_batch_ld = rows n0, the complex64 kernels."""
    x, W, sj = torch_case(batch=3, dtype=torch.float32, wavelet="dog")
    assert W.dtype == torch.complex64 and W.shape == (3, sj.size, 100)
    gW = torch.randn(W.shape, dtype=torch.float32, generator=torch.Generator().manual_seed(1)).to(torch.complex64) * (1 - 1j)
    (gx,) = torch.autograd.grad(W, x, grad_outputs=gW)
    assert gx.dtype == torch.float32 and gx.shape == x.shape
    assert close_to(gx.numpy().astype(np.float64), expected_grad(gW.numpy(), 100, 128, 1 / 4, "dog"), BOUND[32])


def test_two_graphs_alive_on_one_engine(torch_emulated):
    """G.  Two forwards with different dj on the engine of (nfft, precision, device), backpropagated in the opposite order: each
    backward is the transpose of its own forward (ctx.geometry), not of the engine's last call."""
    xa, Wa, _ = torch_case(dj=1 / 4, seed=1)
    xb, Wb, _ = torch_case(dj=1 / 3, seed=2)
    assert Wa.shape[0] != Wb.shape[0]
    (Wb.abs() ** 2).sum().backward()
    (Wa.abs() ** 2).sum().backward()
    assert close_to(xb.grad.numpy(), expected_grad(2 * Wb.detach().numpy(), 100, 128, 1 / 3)[0], 1e-12)
    assert close_to(xa.grad.numpy(), expected_grad(2 * Wa.detach().numpy(), 100, 128, 1 / 4)[0], 1e-12)


def test_backward_uses_the_tolerance_of_its_forward(torch_emulated):
    """G.  pycwt_amd.set_tolerance changed between forward and backward: the gradient has the bits of the run that kept the
    forward's tolerance (and not those of a run at the other one)."""
    import pycwt_amd

    def grad(tol_forward, tol_backward):
        pycwt_amd.set_tolerance(tol_forward)
        x, W, _ = torch_case(n0=3000, dj=1 / 2)
        gW = torch.randn(W.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(torch.complex128)
        pycwt_amd.set_tolerance(tol_backward)
        (g,) = torch.autograd.grad(W, x, grad_outputs=gW)
        return g.numpy()

    kept, changed, other = grad(1e-6, 1e-6), grad(1e-6, None), grad(None, None)
    assert not np.array_equal(kept, other)
    np.testing.assert_array_equal(changed, kept)


def test_non_contiguous_input_and_a_retained_graph(torch_emulated):
    """G.  x given as a strided view: the gradient lands on the view's base through the view; retain_graph = True and a second
    backward give the same bits (the backward keeps no state of its own)."""
    import pycwt_amd
    base = torch.randn(200, dtype=torch.float64, generator=torch.Generator().manual_seed(6), requires_grad=True)
    x = base[::2]
    assert not x.is_contiguous()
    W = pycwt_amd.cwt_torch(x, 1.0, 1 / 4)[0]
    ref = pycwt_amd.cwt_torch(x.detach().contiguous(), 1.0, 1 / 4)[0]
    assert torch.equal(W.detach(), ref)
    loss = (W.abs() ** 2).sum()
    (g1,) = torch.autograd.grad(loss, base, retain_graph=True)
    (g2,) = torch.autograd.grad(loss, base)
    assert torch.equal(g1, g2) and torch.count_nonzero(g1[1::2]) == 0
    assert close_to(g1.numpy()[::2], expected_grad(2 * W.detach().numpy(), 100, 128, 1 / 4)[0], 1e-12)
