"""Shared by tests/test_plan_sequences_emulated.py and tests/test_plan_sequences_gpu.py: call SEQUENCES on one live plan against
fresh plans.  Real callers (the drop-in shim, cwt_torch, the coherence pipeline) keep one plan per (device, length, precision)
alive and push every entry point through it in whatever order the program dictates; the plan carries four LRU row-table slots
with three lazily uploaded device copies each, grow-on-demand scratch shared by unrelated calls, and several invalidation paths.
A stale table or an undersized scratch does not crash: it returns a plausible result for the PREVIOUS call's geometry.

Two judgements per call:
  1. values -- the first time a distinct call is seen, its outputs (of a fresh plan) against the oracle / the closed forms, with
     the bounds that the suite already uses for that output (imported below, none invented: `judge`);
  2. state independence -- the outputs of the call at position i of a sequence on the live plan, padding columns and guard rows
     (prefilled with a sentinel) included, and last_split() equal BIT FOR BIT what the same call returns on a fresh plan with the
     same options and tolerance (memoised per distinct call).

THE CATALOGUE (ENTRIES): every entry point that builds or reads a row table or plan scratch, and the plan state it touches.
`rows_dev` is the device copy of a row-table slot, `adj_dev` / `pool_dev` its derived copies; a key is
[kind, tolerance, mother, parameter, ..., the scales].  NOT part of any key: the output mode (W, power, weighted), hop, pool, n0,
the leading dimensions of the output and of the signals, nbatch of the hop / pool / adjoint calls (they loop over the signals),
the stream.  Part of it: the tolerance, mother and parameter, dt, nrows and every scale, ncols of the calls that hold the
signal, nbatch of the batched calls, xhat_ld of cwt_transform_rows_batch; every option change clears all keys.

  entry                      key kind                          slot copies         plan scratch
  transform, _power, _weighted  0 (with signal, ncols)         rows_dev            xhat (NULL xhat only), band-passed rows xm / xsa
  transform_rows, _rows_power   0 (no signal, ncols)           rows_dev            xm / xsa
  transform_batch, _power, _weighted  3 (nbatch, ncols)        rows_dev            xm / xsa
  transform_rows_batch          2 (nbatch, xhat_ld)            rows_dev            xm / xsa
  transform_hop, _rows_hop      0 (with signal, ncols = n0)    rows_dev            xhat, the fold scratch (rows not fused)
  transform_pool                0 (with signal, ncols = n0)    rows_dev, pool_dev  xhat, the pooled power scratch
  adjoint_rows                  0 (with signal, ncols)         rows_dev, adj_dev   the adjoint's accumulator and row spectra
  adjoint_rows_hop              0 (with signal, ncols = n0)    rows_dev            the same at M points
  adjoint_rows_scales           0 (with signal, ncols = n0)    rows_dev, adj_dev   the same, sgrad_part
  transform_rows_table          never cached: takes the LRU slot and clears its key
  filter_rows                   1 (spec_ld, nrows, a, amp)     rows_dev            xm / xsa
  bluestein (forward_fft_n + transform_rows_n)  its own (a, amp per slab)          bs_* (keyed by n0)
  execute_host, _power          0 (with signal, ncols = n0)    rows_dev            the host staging, xhat

Shapes: nfft = 2^15 with OPTS (the options of the pool and hop tests), where the overlap-save and polynomial forms exist.  TWO
grids hold the forms between them, because the band-passed form is decided per call over all rows: with three rows clipped at
Nyquist they are band-passed rows, with fewer they stay two-pass rows.  Grid A (Morlet 6: ROWS - 1 geometric scales and a third
clipped row) has narrow, overlap-save, band-passed and polynomial rows, grid E (the geometric scales alone, stretched) has the
two-pass rows; ROWS = 15 is the smallest count at which Plan.classify on the emulation shows this in BOTH precisions (at 13
one of the forms is missing; asserted by test_the_grids_hold_every_form).  A single-workgroup row ("small") cannot occur at
nfft > 4096 and narrow_k2048 exists in fp64 only: neither is asked for.  n0 = N - 77 and N 5/8 + 1.  The largest scale has its Fourier period at N / 4 dt.
Bluestein needs nfft >= 2 n0 - 1: n0 = N / 2 - 383 and N / 4 + 809 on the same plan.
"""
import dataclasses
import functools
import hashlib
import math

import numpy as np

import hop_common as hc
import pool_common as pc
import scale_grad_common as sgc
import switch_common as swc
from conftest import row_errors
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_adjoint_emulated import BOUND as ADJOINT_BOUND, numpy_adjoint, rel
from test_kernels_emulated import grid

LOGN = 15
OPTS = {"poly_min_logn": 14, "ols_min_logn": 15}
ROWS = 15
FORMS = ("narrow", "two_pass", "ols", "aols", "poly")
GUARD = 2                                    # rows behind the output that keep the sentinel
SENTINEL = swc.SENTINEL
ALPHA = swc.ALPHA
TOL9 = sgc.TOL9                              # the looser target of the invalidation sequences
EINVAL = -1
SEEDS = (20251, 20252, 20253)                # of the seeded walks


# ---- the arguments of a call -----------------------------------------------------------------------------------------------------
def scales_of(name, N):
    """The scale grids by name.  A: ROWS scales of Morlet(6) from the Fourier period 2 dt to N / 4 dt (bands of eight bins and
    more: the range of scale_grad_common's cases, whose bars are used here), whatever mother the call uses (a change of the mother
    keeps the array).  B ... E: A stretched by a few percent (other tables of about the same
    forms).  E: the geometric rows alone, stretched.  A+ulp, A*1.5: the middle scale moved; A+ulp-first, A+ulp-last, A*1.5-last:
    the first or the last (the ends of the array in a flat key); A-rev; A-trunc: without the last row; A-half: every second."""
    geo = grid(N // 4, 1.0, orc.Mother(orc.MORLET, 6.0), ROWS - 1)
    base = np.sort(np.append(geo, math.sqrt(geo[0] * geo[1])))          # a third row clipped at Nyquist: the band-passed form
    mid = len(base) // 2
    if name in "ABCD":
        return base * {"A": 1.0, "B": 1.03, "C": 1.07, "D": 1.11}[name]
    if name == "E":
        return geo * 1.17                                               # two clipped rows: they stay two-pass rows
    out = base.copy()
    if name == "A+ulp":
        out[mid] = np.nextafter(out[mid], np.inf)
    elif name == "A*1.5":
        out[mid] *= 1.5
    elif name == "A+ulp-first":
        out[0] = np.nextafter(out[0], np.inf)
    elif name == "A+ulp-last":
        out[-1] = np.nextafter(out[-1], 0.0)
    elif name == "A*1.5-last":
        out[-1] /= 1.5
    elif name == "A-rev":
        out = out[::-1].copy()
    elif name == "A-trunc":
        out = out[:-1].copy()
    elif name == "A-half":
        out = out[::2].copy()
    else:
        raise KeyError(name)
    return out


GRIDS = ("A", "B", "C", "D", "E")


def n0_of(N, name, blue=False):
    if blue:
        return {"big": N // 2 - 383, "small": N // 4 + 809}[name]
    return {"big": N - 77, "small": N * 5 // 8 + 1}[name]


@dataclasses.dataclass(frozen=True)
class Call:
    """One call: entry point, mother and parameter, dt, grid, n0, ncols and the padding of the leading dimension, nbatch and the
    padding of x_ld, hop, pool, the output kind of the hop calls (0 W, 1 power, 2 weighted), and the tolerance and options in
    force (beyond the plan's base options; stamped by the runner)."""
    entry: str
    grid: str = "A"
    kind: int = orc.MORLET
    param: float = 6.0
    dt: float = 1.0
    n0: str = "big"
    ncols: str = "n0"             # or "short": 3/4 n0 + 5
    ld_pad: int = 0
    nbatch: int = 1
    x_pad: int = 0
    hop: int = 16
    pool: int = 16
    output: int = 0
    tolerance: float = 0.0
    options: tuple = ()

    def but(self, **kw):
        return dataclasses.replace(self, **kw)

    def __str__(self):
        d = Call(self.entry)
        return "%s(%s)" % (self.entry, ", ".join("%s=%r" % (f.name, getattr(self, f.name)) for f in dataclasses.fields(self)
                                                if f.name != "entry" and getattr(self, f.name) != getattr(d, f.name)))


@dataclasses.dataclass(frozen=True)
class SetTolerance:
    value: float


@dataclasses.dataclass(frozen=True)
class SetOption:
    key: str
    value: int


@dataclasses.dataclass(frozen=True)
class SetStream:
    index: int                    # into the runner's list of streams


@dataclasses.dataclass(frozen=True)
class Refused:
    name: str                     # of REFUSALS


class Context:
    """the resolved arguments and seeded inputs of a call at transform length N"""

    def __init__(self, call, N, prec):
        self.call, self.N, self.prec = call, N, prec
        self.real, self.cplx = hc.types(prec)
        self.kind, self.param, self.dt = call.kind, float(call.param), call.dt
        self.sj = scales_of(call.grid, N)
        self.rows = len(self.sj)
        e = ENTRIES[call.entry]
        self.blue = call.entry == "bluestein"
        self.n0 = n0_of(N, call.n0, self.blue)
        self.nb = call.nbatch if "nbatch" in e.applies else 1
        self.x_ld = self.n0 + (call.x_pad if "nbatch" in e.applies else 0)
        self.ncols = self.n0 * 3 // 4 + 5 if call.ncols == "short" and "ncols" in e.applies else self.n0
        self.hop, self.pool = call.hop * max(1, N >> 16), call.pool      # (16 <= nfft / hop <= 4096: 16 -> 64 at 2^15, 64 -> 256 at 2^18)
        if "hop" in e.applies:
            self.ncols = -(-self.n0 // self.hop)
        if "pool" in e.applies:
            self.ncols = -(-self.n0 // call.pool)
        self.ld = self.ncols + call.ld_pad
        self.output = min(call.output, 1 if call.entry == "transform_rows_hop" else 2) if "output" in e.applies else 0
        self.mother = orc.Mother(self.kind, self.param)

    @functools.cached_property
    def x(self):
        """nb x x_ld: the signals, and the sentinel behind them"""
        rng = np.random.default_rng(1000 + self.n0)
        x = np.full((self.nb, self.x_ld), SENTINEL, dtype=self.real)
        x[:, :self.n0] = rng.standard_normal((self.nb, self.n0)).astype(self.real)
        return x

    @functools.cached_property
    def G(self):
        """nb x rows x ld complex cotangent (the padding columns hold noise too: they must not be read)"""
        rng = np.random.default_rng(2000 + self.n0 + self.rows)
        shape = (self.nb, self.rows, self.ld)
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(self.cplx)

    @functools.cached_property
    def Q(self):
        return swc.draw_q((self.nb * self.rows + GUARD, self.ld), self.real)


def mother_constant(kind, param):
    """conj(psi_ft(f)) = constant x profile(f) (Torrence & Compo 1998, table 1): the amplitudes of cwt_filter_rows"""
    m = int(param)
    if kind == orc.MORLET:
        return complex(math.pi ** -0.25)
    if kind == orc.PAUL:
        return complex(2.0 ** m / math.sqrt(m * math.factorial(2 * m - 1)))
    return complex(np.conj(-(1j ** m)) / math.sqrt(math.gamma(m + 0.5)))


@functools.lru_cache(maxsize=8)
def _bank(N, kind, param, dt, gridname):
    sj = scales_of(gridname, N)
    return orc.filter_bank(sj, orc.angular_freqs(N, dt), N, orc.Mother(kind, param), True)


# ---- one call on a plan: buffers, launch, download ---------------------------------------------------------------------------------
class Job:
    """The device buffers of one call.  prepare (uploads, sentinel fills: these synchronise), launch (the entry point itself:
    nothing but what the ABI does), fetch (every output, then the buffers are freed)."""

    def __init__(self, lib, plan, call, N, prec):
        self.lib, self.plan, self.call = lib, plan, call
        self.c = Context(call, N, prec)
        self.bufs, self.outs, self.host = [], [], {}
        self.go = ENTRIES[call.entry].prepare(self, self.c)
        self.split = None

    def up(self, a):
        a = np.ascontiguousarray(a)
        b = _hip.DeviceBuffer(max(a.nbytes, 16), lib=self.lib)
        self.bufs.append(b)
        b.upload(self.plan, a)
        return b

    def out(self, name, shape, dtype):
        fill = SENTINEL * (1 + 1j) if np.dtype(dtype).kind == "c" else SENTINEL
        b = self.up(np.full(shape, fill, dtype=dtype))
        self.outs.append((name, b, shape, dtype))
        return b

    def launch(self):
        self.go(self.plan)
        self.split = self.plan.last_split()

    def fetch(self):
        res = {name: b.download(self.plan, shape, dtype) for name, b, shape, dtype in self.outs}
        res.update(self.host)
        self.free()
        return res

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _x1(j, c):
    return j.up(c.x[0, :c.n0])


def _out_rows(j, c, real=False, name="W"):
    return j.out(name, (c.nb * c.rows + GUARD, c.ld), c.real if real else c.cplx)


def _p_transform(power=0, weighted=False):
    def prepare(j, c):
        x, xh, W = _x1(j, c), j.out("xhat", (c.N,), c.cplx), _out_rows(j, c, real=power)
        Q = j.up(c.Q) if weighted else None
        args = (x.ptr, c.n0, c.kind, c.param, c.dt, c.sj, xh.ptr)

        def go(p):
            if weighted:
                p.transform_weighted(*args, Q.ptr, ALPHA, W.ptr, c.ld, c.ncols)
            else:
                (p.transform_power if power else p.transform)(*args, W.ptr, c.ld, c.ncols)
        return go
    return prepare


def _p_transform_rows(power=0):
    def prepare(j, c):
        x, xh, W = _x1(j, c), j.out("xhat", (c.N,), c.cplx), _out_rows(j, c, real=power)

        def go(p):
            p.forward_fft(x.ptr, c.n0, xh.ptr)
            (p.transform_rows_power if power else p.transform_rows)(xh.ptr, c.kind, c.param, c.dt, c.sj, W.ptr, c.ld, c.ncols)
        return go
    return prepare


def _p_batch(power=0, weighted=False, from_spectra=False):
    def prepare(j, c):
        x, xh, W = j.up(c.x), j.out("xhat", (c.nb, c.N), c.cplx), _out_rows(j, c, real=power)
        Q = j.up(c.Q) if weighted else None
        args = (x.ptr, c.nb, c.x_ld, c.n0, c.kind, c.param, c.dt, c.sj, xh.ptr)

        def go(p):
            if from_spectra:
                p.fft_rows(x.ptr, False, c.nb, c.x_ld, c.n0, xh.ptr)
                p.transform_rows_batch(xh.ptr, c.nb, c.N, c.kind, c.param, c.dt, c.sj, W.ptr, c.ld, c.ncols)
            elif weighted:
                p.transform_batch_weighted(*args, Q.ptr, ALPHA, W.ptr, c.ld, c.ncols)
            else:
                (p.transform_batch_power if power else p.transform_batch)(*args, W.ptr, c.ld, c.ncols)
        return go
    return prepare


def _p_hop(from_spectra=False):
    def prepare(j, c):
        output = c.output
        x, xh, W = j.up(c.x), j.out("xhat", (c.nb, c.N), c.cplx), _out_rows(j, c, real=output == 1)
        Q = j.up(c.Q) if output == 2 else None

        def go(p):
            if from_spectra:
                p.fft_rows(x.ptr, False, c.nb, c.x_ld, c.n0, xh.ptr)
                p.transform_rows_hop(xh.ptr, c.nb, c.N, c.n0, c.kind, c.param, c.dt, c.sj, c.hop, output, W.ptr, c.ld)
            else:
                p.transform_hop(x.ptr, c.nb, c.x_ld, c.n0, c.kind, c.param, c.dt, c.sj, c.hop, xh.ptr, output, W.ptr, c.ld,
                                Q.ptr if Q else None, ALPHA)
        return go
    return prepare


def _p_pool(j, c):
    x, xh, P = j.up(c.x), j.out("xhat", (c.nb, c.N), c.cplx), _out_rows(j, c, real=True, name="P")

    def go(p):
        p.transform_pool(x.ptr, c.nb, c.x_ld, c.n0, c.kind, c.param, c.dt, c.sj, c.pool, xh.ptr, P.ptr, c.ld)
    return go


def _p_adjoint(hop=False):
    def prepare(j, c):
        G = j.up(c.G)
        cols = c.n0 if hop else c.ncols                              # (the columns of xbar)
        xb = j.out("xbar", (c.nb, cols + c.call.x_pad), c.real)

        def go(p):
            if hop:
                p.adjoint_rows_hop(G.ptr, c.nb, c.rows * c.ld, c.ld, c.hop, c.n0, c.kind, c.param, c.dt, c.sj, xb.ptr, cols + c.call.x_pad)
            else:
                p.adjoint_rows(G.ptr, c.nb, c.rows * c.ld, c.ld, cols, c.kind, c.param, c.dt, c.sj, xb.ptr, cols + c.call.x_pad)
        return go
    return prepare


def _p_scales(j, c):
    x, xh, G = j.up(c.x), j.out("xhat", (c.nb, c.N), c.cplx), j.up(c.G)
    xb, sg = j.out("xbar", (c.nb, c.n0 + c.call.x_pad), c.real), j.out("sgrad", (c.rows + 1, 2), np.float64)

    def go(p):
        p.fft_rows(x.ptr, False, c.nb, c.x_ld, c.n0, xh.ptr)
        p.adjoint_rows_scales(G.ptr, c.nb, c.rows * c.ld, c.ld, 1, c.n0, xh.ptr, c.N, c.kind, c.param, c.dt, c.sj, xb.ptr,
                              c.n0 + c.call.x_pad, sg.ptr)
    return go


def _p_table(j, c):
    bank = _bank(c.N, c.kind, c.param, c.dt, c.call.grid).astype(c.cplx)
    x, xh, W, tab = _x1(j, c), j.out("xhat", (c.N,), c.cplx), _out_rows(j, c), j.up(bank)
    k_lo, nband = np.full(c.rows, -(c.N // 2), dtype=np.int32), np.full(c.rows, c.N, dtype=np.int32)

    def go(p):
        p.forward_fft(x.ptr, c.n0, xh.ptr)
        p.transform_rows_table(xh.ptr, tab.ptr, k_lo, nband, W.ptr, c.ld, c.ncols)
    return go


def _p_filter(j, c):
    x, xh, W = _x1(j, c), j.out("xhat", (c.N,), c.cplx), _out_rows(j, c)
    w1 = 2.0 * math.pi / (c.N * c.dt)
    a, amp = c.sj * w1, np.sqrt(c.sj * w1 * c.N) * mother_constant(c.kind, c.param)

    def go(p):
        p.forward_fft(x.ptr, c.n0, xh.ptr)
        p.filter_rows(xh.ptr, 0, c.kind, c.param, a, amp, W.ptr, c.ld, c.ncols)
    return go


def _p_bluestein(j, c):
    x, xh, W = _x1(j, c), j.out("xhat", (c.n0,), c.cplx), _out_rows(j, c)

    def go(p):
        p.forward_fft_n(x.ptr, c.n0, xh.ptr)
        p.transform_rows_n(xh.ptr, c.n0, c.kind, c.param, c.dt, c.sj, W.ptr, c.ld)
    return go


def _p_host(power=0):
    def prepare(j, c):
        def go(p):
            W, xhat = (p.execute_host_power if power else p.execute_host)(c.x[0, :c.n0], c.kind, c.param, c.dt, c.sj)
            j.host = {"W": np.array(W), "xhat": xhat}
        return go
    return prepare


@dataclasses.dataclass(frozen=True)
class Entry:
    prepare: object
    applies: frozenset            # the arguments of Call that the entry point has, beyond mother, dt, grid and n0
    out: str                      # what `judge` compares the main output with
    synchronises: bool = False    # the host-buffer calls


def _e(prepare, applies, out, **kw):
    return Entry(prepare, frozenset(applies.split()), out, **kw)


ENTRIES = {
    "transform": _e(_p_transform(), "ncols ld", "W"),
    "transform_rows": _e(_p_transform_rows(), "ncols ld", "W"),
    "transform_power": _e(_p_transform(power=1), "ncols ld", "power"),
    "transform_rows_power": _e(_p_transform_rows(power=1), "ncols ld", "power"),
    "transform_weighted": _e(_p_transform(weighted=True), "ncols ld", "weighted"),
    "transform_batch": _e(_p_batch(), "ncols ld nbatch", "W"),
    "transform_rows_batch": _e(_p_batch(from_spectra=True), "ncols ld nbatch", "W"),
    "transform_batch_power": _e(_p_batch(power=1), "ncols ld nbatch", "power"),
    "transform_batch_weighted": _e(_p_batch(weighted=True), "ncols ld nbatch", "weighted"),
    "transform_hop": _e(_p_hop(), "ld nbatch hop output", "hop"),
    "transform_rows_hop": _e(_p_hop(from_spectra=True), "ld nbatch hop output", "hop"),
    "transform_pool": _e(_p_pool, "ld nbatch pool", "pool"),
    "adjoint_rows": _e(_p_adjoint(), "ncols ld nbatch", "adjoint"),
    "adjoint_rows_hop": _e(_p_adjoint(hop=True), "ld nbatch hop", "adjoint"),
    "adjoint_rows_scales": _e(_p_scales, "ld nbatch", "scales"),
    "transform_rows_table": _e(_p_table, "ncols ld", "W"),
    "filter_rows": _e(_p_filter, "ncols ld", "W"),
    "bluestein": _e(_p_bluestein, "ld", "W"),
    "execute_host": _e(_p_host(), "", "W", synchronises=True),
    "execute_host_power": _e(_p_host(power=1), "", "power", synchronises=True),
}
NAMES = tuple(ENTRIES)
POW2_NAMES = tuple(n for n in NAMES if n != "bluestein")       # Bluestein mixes with these in sequences of its own


# ---- refused calls ----------------------------------------------------------------------------------------------------------------
def _refusals():
    """name -> f(plan, scratch pointer, scales of A, N): each refused with CWT_EINVAL before anything is queued (the refusal lists
    of test_pool_emulated, test_scale_grad_emulated and test_exports_edges), and one refused for its row count with the
    arguments -- grid A -- of a call whose table is in the cache.  "a scale of 0" is refused AFTER the lookup has taken the
    least recently used slot and cleared its key (prepare_table checks the scales while it builds the rows): the one refusal
    that leaves a trace in the cache.  One scratch buffer (REFUSAL_BYTES) stands for every pointer; it holds the largest call
    that any of these WOULD be, were it not refused."""
    M = orc.MORLET

    def n0(N):
        return N - 77
    def holed(sj):
        out = np.array(sj)
        out[len(out) // 2] = 0.0
        return out
    return {
        "a scale of 0": lambda p, B, sj, N: p.transform(B, n0(N), M, 6.0, 1.0, holed(sj), None, B, n0(N), n0(N)),
        "pool not a power of two": lambda p, B, sj, N: p.transform_pool(B, 1, n0(N), n0(N), M, 6.0, 1.0, sj, 12, None, B, n0(N)),
        "pool: ldp < ncols_p": lambda p, B, sj, N: p.transform_pool(B, 1, n0(N), n0(N), M, 6.0, 1.0, sj, 16, None, B, 5),
        "hop: nfft / hop > 4096": lambda p, B, sj, N: p.transform_hop(B, 1, n0(N), n0(N), M, 6.0, 1.0, sj, 2, None, 0, B, n0(N)),
        "scales: xhat NULL": lambda p, B, sj, N: p.adjoint_rows_scales(B, 1, len(sj) * n0(N), n0(N), 1, n0(N), None, N, M, 6.0, 1.0, sj,
                                                                      B, n0(N), B),
        "adjoint: a filter bank": lambda p, B, sj, N: p.adjoint_rows(B, 1, len(sj) * n0(N), n0(N), n0(N), 3, 0.0, 1.0, sj, B, n0(N)),
        "transform: ldw < ncols": lambda p, B, sj, N: p.transform(B, n0(N), M, 6.0, 1.0, sj, None, B, n0(N) - 1, n0(N)),
        "filter_rows: 0 < spec_ld < nfft": lambda p, B, sj, N: p.filter_rows(B, 8, _hip.DOG, 0.0, sj, 1.0, B, n0(N), n0(N)),
        "forward_fft_n: nfft < 2 n0 - 1": lambda p, B, sj, N: p.forward_fft_n(B, N // 2 + 1, B),
        "rows > max_rows": lambda p, B, sj, N: p.transform_batch(B, p.max_rows // len(sj) + 1, n0(N), n0(N), M, 6.0, 1.0, sj, B, B,
                                                                n0(N), n0(N)),
    }


REFUSALS = _refusals()


def refusal_bytes(N, max_rows):
    """"rows > max_rows" is the largest: max_rows + ROWS rows of N complex128 columns at the most"""
    return (max_rows + ROWS) * N * 16 + 64


# ---- judgement 1: values ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=12)
def _oracle(N, kind, param, dt, gridname, n0name, nb, prec, blue):
    """the oracle's rows of every signal of the call (nb x rows x n0 complex128), read-only"""
    c = Context(Call("bluestein" if blue else "transform_batch", gridname, kind, param, dt, n0name, nbatch=nb), N, prec)
    W = np.stack([orc.cwt_rows(c.x[b, :c.n0].astype(np.float64), dt, c.sj, c.mother, N=c.n0 if blue else N)[:, :c.n0]
                  for b in range(c.nb)])
    W.flags.writeable = False
    return W


def w_bound(wtol, prec, target):
    """per row max|dW| / the row's peak: the backend's round-off bound (test_kernels_emulated.TOL on the emulation,
    test_gpu_parity.TOL on the GPU), or the target itself (tests/test_switch_scales_emulated.bound_of)"""
    return max(target, wtol[prec])


def judge(call, res, N, prec, wtol):
    """Asserts the outputs `res` of `call` against the truth, each with the bound the suite already has for it:
      W         conftest.row_errors against the oracle, w_bound
      xhat      against np.fft.fft, relative to its largest bin, the round-off bound of W (test_kernels_emulated.run_case)
      power     against the oracle's |W|^2 per row relative to the row's peak power, 2 x w_bound (pool_common.ORACLE_BOUND's
                reasoning: d|W|^2 = 2 |W| d|W|)
      weighted  against (alpha Q) x the oracle's W, per row relative to max|alpha Q| x the row's peak: |alpha Q| |dW|, w_bound
      hop       hop_common.row_error against the oracle's columns ::hop, max(target, hop_common.HOP_BOUND); its power and weighted
                outputs as above with that bound in the place of w_bound
      pool      pool_common.row_ratio against pool_common.window_means of the oracle's power, max(2 target, pool_common.ORACLE_BOUND)
      adjoint   test_adjoint_emulated.rel against numpy_adjoint, max(10 target, test_adjoint_emulated.BOUND) -- the rule of
                test_polynomial_transpose_agrees_with_the_general_path
      scales    scale_grad_common.ratio against its closed form, BAR (round-off) or BAR_TOL9 (1e-9, fp64); xbar as adjoint
    The padding columns and guard rows hold the sentinel."""
    c = Context(call, N, prec)
    e = ENTRIES[call.entry]
    target = call.tolerance
    wb = w_bound(wtol, prec, target)
    ref = _oracle(N, c.kind, c.param, c.dt, call.grid, call.n0, c.nb, prec, c.blue)            # nb x rows x n0
    live = c.nb * c.rows
    what = str(call)
    if "xhat" in res:
        n = c.n0 if c.blue else c.N
        xh = np.asarray(res["xhat"]).reshape(-1, n).astype(np.complex128)
        for b in range(xh.shape[0]):
            xref = np.fft.fft(c.x[b, :c.n0].astype(np.float64), n=n)
            assert np.abs(xh[b] - xref).max() <= wtol[prec] * np.abs(xref).max(), (what, "xhat", b)
    if e.out in ("W", "power", "weighted", "hop", "pool"):
        key = "P" if e.out == "pool" else "W"
        out = np.asarray(res[key])
        if not e.synchronises:
            assert out.shape == (live + GUARD, c.ld), (what, out.shape)
            fill = SENTINEL * (1 + 1j) if out.dtype.kind == "c" else SENTINEL
            assert np.all(out[live:] == fill) and np.all(out[:live, c.ncols:] == fill), (what, "wrote outside its output")
        got = out[:live, :c.ncols].reshape(c.nb, c.rows, c.ncols)
        peak = np.abs(ref).max(axis=2)                                                          # nb x rows
        kind_out = e.out if e.out != "hop" else ("hop", "power", "weighted")[c.output]
        hb = max(target, hc.HOP_BOUND[prec])
        for b in range(c.nb):
            if e.out == "pool":
                means = pc.window_means(ref[b].real ** 2 + ref[b].imag ** 2, c.pool)
                err = pc.row_ratio(got[b], means).max()
                bound = max(2 * target, pc.ORACLE_BOUND[prec])
            else:
                step = c.hop if e.out == "hop" else 1
                r = ref[b][:, ::step][:, :c.ncols]
                base = hb if e.out == "hop" else wb
                if kind_out in ("W", "hop"):
                    err = hc.row_error(got[b], r, peak[b]) if e.out == "hop" else row_errors(got[b], r)[0].max()
                    bound = base
                elif kind_out == "power":
                    err = (np.abs(got[b].astype(np.float64) - (r.real ** 2 + r.imag ** 2)).max(axis=1) / peak[b] ** 2).max()
                    bound = 2 * base
                else:
                    q = ALPHA * c.Q[:live, :c.ncols].reshape(c.nb, c.rows, c.ncols)[b].astype(np.float64)
                    err = (np.abs(got[b].astype(np.complex128) - q * r).max(axis=1) / (np.abs(q).max(axis=1) * peak[b])).max()
                    bound = base
            assert err <= bound, (what, e.out, kind_out, b, float(err), bound)
    if e.out in ("adjoint", "scales"):
        hop = c.hop if call.entry == "adjoint_rows_hop" else 1
        cols = c.n0 if call.entry != "adjoint_rows" else c.ncols
        xb = np.asarray(res["xbar"])
        assert np.all(xb[:, cols:] == SENTINEL), (what, "xbar wrote outside its output")
        nch = -(-c.n0 // hop) if hop > 1 else cols
        for b in range(c.nb):
            Gb = c.G[b, :, :nch].astype(np.complex128)
            full = np.zeros((c.rows, cols), dtype=np.complex128)
            full[:, ::hop] = Gb
            want = numpy_adjoint(full, c.sj / c.dt, c.mother, c.N)          # ((s, dt) is (s / dt, 1) to the filter bank)
            err, bound = rel(xb[b, :cols].astype(np.float64), want), max(10 * target, ADJOINT_BOUND[prec])
            assert err <= bound, (what, "xbar", b, err, bound)
    if e.out == "scales":
        sg = np.asarray(res["sgrad"])
        assert np.all(sg[c.rows:] == SENTINEL), (what, "sgrad wrote outside its output")
        want, S = np.zeros((c.rows, 2)), np.zeros((c.rows, 2))
        for b in range(c.nb):
            w, s = sgc.reference(c.kind, c.param, c.sj, c.x[b, :c.n0], c.G[b, :, :c.n0], c.N, 1, c.dt)
            want, S = want + w, S + s
        assert target in (0.0, TOL9), target
        bar = sgc.BAR[prec] if target <= (1e-16 if prec == 64 else 1e-8) else max(sgc.BAR[prec], sgc.BAR_TOL9)
        err = sgc.ratio(sg[:c.rows], want, S)
        assert err <= bar, (what, "sgrad", err, bar)


# ---- judgement 2: the runner --------------------------------------------------------------------------------------------------------
def bits(res):
    """{name: (shape, dtype, a digest of the bytes)} of the outputs of a call: what two plans must agree in"""
    return {k: (np.shape(v), str(np.asarray(v).dtype), hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).digest())
            for k, v in res.items()}


# the defaults of the options that the sequences toggle (include/cwt_hip.h): a call made after the return to a default is the
# call of a fresh plan without the option
DEFAULTS = {("adjoint_poly", 64): 1, ("adjoint_poly", 32): 1, ("hop_fuse_terms", 64): 1, ("hop_fuse_terms", 32): 1, ("poly", 64): 1,
            ("poly", 32): 1, ("serial_rows", 64): 2, ("serial_rows", 32): 0}


class Runner:
    """Runs sequences on live plans of one (library, nfft, precision) and compares every call with a fresh plan's (memoised for
    the life of the runner -- one per test module, length and precision -- as digests of the bytes).  wtol: the backend's
    round-off bound on W per precision."""

    def __init__(self, lib, N, prec, wtol, options=OPTS, streams=None, values=True):
        self.lib, self.N, self.prec, self.wtol = lib, N, prec, wtol
        self.base = dict(options or {})
        self.max_rows = 3 * ROWS
        self.streams = streams or []
        self.values = values
        self.memo = {}

    def plan(self, tolerance=0.0, options=()):
        opts = dict(self.base)
        opts.update(dict(options))
        plan = _hip.Plan(self.N, self.prec, max_rows=self.max_rows, lib=self.lib, options=opts)
        if tolerance:
            plan.set_tolerance(tolerance)
        return plan

    def fresh(self, call):
        """(bits of the outputs, last_split) of the call as the first call of a new plan; judged against the truth when first made"""
        if call not in self.memo:
            plan = self.plan(call.tolerance, call.options)
            try:
                job = Job(self.lib, plan, call, self.N, self.prec)
                try:
                    job.launch()
                    res = job.fetch()
                finally:
                    job.free()
            finally:
                plan.close()
            if self.values:
                judge(call, res, self.N, self.prec, self.wtol)
            self.memo[call] = (bits(res), job.split)
        return self.memo[call]

    def stamp(self, steps):
        """the steps with the tolerance and the options in force written into every call"""
        tol, opts, out = 0.0, {}, []
        for s in steps:
            if isinstance(s, SetTolerance):
                tol = s.value
            elif isinstance(s, SetOption):
                opts[s.key] = s.value
                if s.value == self.base.get(s.key, DEFAULTS[s.key, self.prec]):
                    del opts[s.key]
            out.append(s.but(tolerance=tol, options=tuple(sorted(opts.items()))) if isinstance(s, Call) else s)
        return out

    def run(self, steps, name, back_to_back=False):
        """One live plan through `steps` (Call, SetTolerance, SetOption, SetStream, Refused).  back_to_back: the inputs of every
        call are uploaded first, the calls then follow each other with no host synchronisation but the ABI's own, and the
        outputs -- distinct buffers -- are downloaded at the end.  Returns the number of calls made."""
        stamped = self.stamp(list(steps))
        listing = "\n".join("  %3d  %s" % (i, s) for i, s in enumerate(stamped))

        def check(i, s, job):
            got, (want, split) = bits(job.fetch()), self.fresh(s)
            bad = [k for k in want if got.get(k) != want[k]]
            if job.split != split:
                bad.append("last_split %s != %s" % (job.split, split))
            assert not bad, "%s (nfft %d, precision %d): call %d, %s, differs from a fresh plan's in %s\n%s" % (
                name, self.N, self.prec, i, s, bad, listing)
        plan = self.plan()
        jobs, scratch, made = {}, None, 0
        try:
            if any(isinstance(s, Refused) for s in stamped):
                scratch = _hip.DeviceBuffer(refusal_bytes(self.N, self.max_rows), lib=self.lib)
            if back_to_back:
                jobs = {i: Job(self.lib, plan, s, self.N, self.prec) for i, s in enumerate(stamped) if isinstance(s, Call)}
            last = None
            for i, s in enumerate(stamped):
                if isinstance(s, SetTolerance):
                    plan.set_tolerance(s.value)
                elif isinstance(s, SetOption):
                    plan.set_option(s.key, s.value)
                elif isinstance(s, SetStream):
                    plan.set_stream(self.streams[s.index])
                elif isinstance(s, Refused):
                    try:
                        REFUSALS[s.name](plan, scratch.ptr, scales_of("A", self.N), self.N)
                    except _hip.HipError as err:
                        assert err.code == EINVAL, (name, i, s, err)
                    else:
                        raise AssertionError("%s: step %d (%s) was not refused\n%s" % (name, i, s.name, listing))
                    assert last is None or plan.last_split() == last, "%s: step %d (refused: %s) changed last_split()\n%s" % (
                        name, i, s.name, listing)
                else:
                    job = jobs[i] if back_to_back else Job(self.lib, plan, s, self.N, self.prec)
                    jobs[i] = job
                    job.launch()
                    last = job.split
                    made += 1
                    if not back_to_back:
                        check(i, s, job)
                        del jobs[i]
            for i in sorted(jobs):
                check(i, stamped[i], jobs[i])
        finally:
            for job in jobs.values():
                job.free()
            if scratch is not None:
                scratch.free()
            plan.close()
        return made


# ---- the sequences -----------------------------------------------------------------------------------------------------------------
def variations(entry):
    """(a): the base call of `entry` on grid A and every call that differs from it in exactly ONE argument the entry point has"""
    base = Call(entry)
    has = ENTRIES[entry].applies
    out = [base.but(n0="small"), base.but(dt=0.5), base.but(param=5.5), base.but(kind=orc.DOG, param=2.0),
           base.but(grid="A+ulp"), base.but(grid="A*1.5"), base.but(grid="A+ulp-first"), base.but(grid="A+ulp-last"),
           base.but(grid="A*1.5-last"), base.but(grid="A-rev"), base.but(grid="A-trunc")]
    if "ncols" in has:
        out.append(base.but(ncols="short"))
    if "ld" in has:
        out.append(base.but(ld_pad=3))
    if "nbatch" in has:
        out.append(base.but(nbatch=3, x_pad=5))
    if "hop" in has:
        out.append(base.but(hop=64))
    if "pool" in has:
        out.append(base.but(pool=64))
    if "output" in has:
        out += [base.but(output=1)] + ([base.but(output=2)] if entry == "transform_hop" else [])
    return base, out


def seq_one_argument(entry, part=None):
    """transform(A), then E(A), E(one argument changed), E(A) for every argument: the base form before and after each change.
    part = (k, n): every n-th variation from the k-th (the long transforms of the GPU module, a few seconds per case)"""
    base, var = variations(entry)
    if part is not None:
        var = var[part[0]::part[1]]
    steps = [Call("transform"), base]
    for v in var:
        steps += [v, base]
    return steps


def pair_walk(names):
    """A closed walk in which every ORDERED pair of `names` (a name with itself included) occurs consecutively exactly once: an
    Euler circuit of the complete directed graph with loops (Hierholzer), len(names)^2 + 1 calls."""
    n = len(names)
    nxt = [0] * n
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append((v + nxt[v]) % n)           # (edge v -> v + k, k = 0 ... n - 1)
            nxt[v] += 1
        else:
            circuit.append(stack.pop())
    return [names[i] for i in reversed(circuit)]


def pairs_of(walk):
    return set(zip(walk[:-1], walk[1:]))


def seq_pairs(names=POW2_NAMES, grid="A"):
    walk = pair_walk(list(names))
    assert pairs_of(walk) == {(a, b) for a in names for b in names}, "the walk misses ordered pairs"
    return [Call(e, grid) for e in walk]


def segments(steps, n):
    """`steps` cut into n consecutive pieces, each beginning with the last step of the one before: every consecutive pair of
    `steps` is a consecutive pair of exactly one piece"""
    size = -(-(len(steps) - 1) // n)
    out = [steps[i * size:(i + 1) * size + 1] for i in range(n)]
    assert sum(len(p) - 1 for p in out) == len(steps) - 1 and all(len(p) > 1 for p in out)
    return out


def seq_eviction(derived, other="adjoint_rows"):
    """(c): five grids on four slots.  `derived`(A) and `other`(A) upload the slot's derived copies, transforms of B ... E evict the
    slot, then both again; and `derived` alone through A ... E, A."""
    first = [Call(derived), Call(other)] + [Call("transform", g) for g in "BCDE"] + [Call(derived), Call(other)]
    second = [Call(derived, g) for g in "ABCDE"] + [Call(derived)]
    return first, second


EVICTION_PAIRS = (("transform_pool", "adjoint_rows"), ("adjoint_rows_scales", "transform_pool"), ("transform_hop", "adjoint_rows"),
                  ("adjoint_rows", "transform_pool"))

TOGGLES = ("tolerance", "adjoint_poly", "hop_fuse_terms", "poly", "serial_rows")
BLUESTEIN_MIX = ("bluestein", "transform", "transform_pool", "adjoint_rows_scales", "transform_hop", "execute_host")


def toggle_steps(toggle, prec):
    """(the step that leaves the first state, the step that returns to it)"""
    if toggle == "tolerance":
        return SetTolerance(TOL9), SetTolerance(0.0)
    first = DEFAULTS[toggle, prec]
    return SetOption(toggle, 0 if first else 2), SetOption(toggle, first)


def seq_invalidation(toggle, prec, every=7):
    """(d): the walk of (b) with the change before every `every`-th call, away and back in turn (7 and the 19 entry points are
    coprime: every entry point meets both states after many predecessors), and a return to the first state at the end"""
    away, back = toggle_steps(toggle, prec)
    steps, state = [], 0
    for i, c in enumerate(seq_pairs()):
        if i and i % every == 0:
            state ^= 1
            steps.append(away if state else back)
        steps.append(c)
    if state:
        steps.append(back)
    return steps + [Call(e) for e in POW2_NAMES[:3]]


SCRATCH = {                       # (e): entry -> the options in force
    "transform_pool": {},
    "transform_hop": {"hop_fuse_terms": 0},
    "adjoint_rows_scales": {},
    "transform": {},                                           # the band-passed rows' xm / xsa
    "transform_batch": {},
    "bluestein": {},
    "execute_host": {},
}


def seq_scratch(entry):
    """(e): [(name, small-large-small, large-small-large)]: small and large differ in n0, in the rows, in nbatch, one at a time"""
    batched = "nbatch" in ENTRIES[entry].applies
    big = Call(entry, nbatch=3 if batched else 1)
    dims = [("n0", big.but(n0="small")), ("rows", big.but(grid="A-half"))] + ([("nbatch", big.but(nbatch=1))] if batched else [])
    pre = [SetOption(k, v) for k, v in SCRATCH[entry].items()]
    return [(d, pre + [small, big, small], pre + [big, small, big]) for d, small in dims]


def seq_refusals():
    """(f): the walk of (b) with one refused call between any two, the refusals in turn"""
    calls, refused = seq_pairs(), list(REFUSALS)
    steps = []
    for i, c in enumerate(calls[:-1]):
        steps += [c, Refused(refused[i % len(refused)])]
    return steps + [calls[-1]]


def seq_refusal_after_lookup():
    """(f): the refusal that comes after the lookup took a slot, placed so that the slot it takes is the one the next call needs
    (A's, with its pool_dev and adj_dev copies: the four slots hold A, B, C, D and A is the least recently used) and then one that
    the next call does not need (B's, before calls on D and C; B itself follows)"""
    zero = Refused("a scale of 0")
    return ([Call("transform_pool"), Call("adjoint_rows")] + [Call("transform", g) for g in "BCD"] + [zero, Call("transform_pool"),
            Call("adjoint_rows"), zero, Call("transform", "D"), Call("transform", "C"), Call("transform", "B"), zero, zero,
            Call("transform_pool"), Call("transform", "B")])


def seq_walk(seed, prec, length=40):
    """(g): `length` steps drawn from the whole catalogue: entry points x grids A ... E x the two n0, and -- one step in eight --
    a change of the tolerance or of an option"""
    rng = np.random.default_rng(seed)
    changes = [SetTolerance(TOL9), SetTolerance(0.0)] + [s for t in ("adjoint_poly", "hop_fuse_terms", "poly", "serial_rows")
                                                          for s in toggle_steps(t, prec)]
    steps = []
    for _ in range(length):
        if rng.random() < 0.125:
            steps.append(changes[int(rng.integers(len(changes)))])
        else:
            steps.append(Call(NAMES[int(rng.integers(len(NAMES)))], grid=GRIDS[int(rng.integers(len(GRIDS)))],
                              n0=("big", "small")[int(rng.integers(2))]))
    return steps


def base_split(lib, N, prec, options=OPTS, name="A"):
    """last_split() of transform(grid `name`) at round-off, by Plan.classify alone (nothing is launched)"""
    plan = _hip.Plan(N, prec, max_rows=3 * ROWS, lib=lib, options=options)
    try:
        labels = plan.classify(orc.MORLET, 6.0, 1.0, scales_of(name, N), N - 77, True)
    finally:
        plan.close()
    kinds = [lab.split("/")[0] for lab in labels]
    return {f: sum(k == f or (f == "narrow" and k.startswith("narrow")) or (f == "ols" and k.startswith("ols")) for k in kinds)
            for f in FORMS}
