"""Shared by test_poly_xcd_emulated.py and test_poly_xcd_gpu.py: k_poly_rows under the XCD-local mapping of its workgroups (plan
option poly_xcd = 1, the default) against the mapping piece = blockIdx.x (poly_xcd = 0), BIT FOR BIT, through every entry point that
launches the kernel: the complex output (cwt_transform), the power output (cwt_transform_power) and the weighted output
(cwt_transform_weighted).  The remap only changes which workgroup computes which 8 KB piece of a row, so nothing but equality of
the bits is acceptable.  The outputs are prefilled with a sentinel and compared whole, padding columns included: equal buffers
also mean that every piece of every row was written under the new mapping (the remap is a bijection of the grid) and nothing else.

Shapes: N = 2^16 is the shortest transform with polynomial rows; eight scales of a 256-row Morlet(6) grid chosen so that, at the
accuracy target 1e-9, intervals K' = 256, 512, 1024 and degrees 4, 6, 8 all occur in both precisions (checked, not assumed).  The
workgroup grid of a row has ceil(ncols / 512) (complex128) or ceil(ncols / 1024) (complex64) pieces; a group of the remap is 8
stretches of 32 pieces, and a row's last group of m < 256 pieces gives m % 8 stretches one piece more than the others:
    ncols = N, N - 1   128 / 64 pieces: one short group, stretches of 16 / 8
    ncols = 12345      25 / 13 pieces: not a multiple of 8 (stretches of 4 and 3 / 2 and 1), a ragged last piece
    ncols = 40000      79 / 40 pieces
    N = 2^18, ncols = N - 1000: 511 pieces = a whole group and one of 255 (complex128), 256 = exactly one whole group (complex64)
    N = 2^20 (GPU only): 2048 pieces, eight whole groups -- the flagship's grid.
"""
import numpy as np

from pycwt_amd import _hip

MORLET, F0 = 0, 6.0
TOLERANCE = 1e-9
IDX = [106, 118, 123, 135, 141, 170, 220, 250]          # rows of the 256-scale grid at N = 2^16
WANT = {(1024, 8), (1024, 6), (512, 8), (512, 6), (256, 8), (256, 6), (256, 4)}
SENTINEL = -7.0
ALPHA = -0.75


def scales(N, idx, rows=256):
    flambda = 4 * np.pi / (F0 + np.sqrt(2 + F0 * F0))
    s0 = 2.0 / flambda
    dj = np.log2(N / s0) / (rows - 1)
    return (s0 * 2 ** (np.arange(rows) * dj))[list(idx)]


def kd_of(label):
    """'poly/K1024/d8' -> (1024, 8)"""
    _, k, d = label.split("/")
    return int(k[1:]), int(d[1:])


def outputs(lib, N, prec, sj, ncols, xcd, ld_pad=3, extra=None):
    """{'W', 'power', 'weighted'}: the whole rows x (ncols + ld_pad) buffers after one call each on one plan, the row classes and
    the number of k_poly_rows launches per call (= plane chunks; option profile)."""
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    rows, ld = len(sj), ncols + ld_pad
    plan = _hip.Plan(N, prec, max_rows=rows, lib=lib, options=dict(extra or {}, poly_xcd=xcd, profile=1))
    plan.set_tolerance(TOLERANCE)
    bufs = []

    def up(a):
        b = _hip.DeviceBuffer(a.nbytes, lib=lib)
        bufs.append(b)
        b.upload(plan, np.ascontiguousarray(a))
        return b
    try:
        rng = np.random.default_rng(5)
        x = rng.standard_normal(ncols).astype(real)
        Q = rng.standard_normal((rows, ld)).astype(real)
        xd, xh, Qd = up(x), up(np.zeros(N, dtype=cplx)), up(Q)
        Wd = up(np.full((rows, ld), SENTINEL * (1 + 1j), dtype=cplx))
        Pd = up(np.full((rows, ld), SENTINEL, dtype=real))
        Gd = up(np.full((rows, ld), SENTINEL * (1 + 1j), dtype=cplx))
        plan.sync()
        plan.timings()
        plan.transform(xd.ptr, ncols, MORLET, F0, 1.0, sj, xh.ptr, Wd.ptr, ld, ncols)
        plan.sync()
        chunks = plan.timings()["poly"][1]
        classes = plan.row_classes()
        plan.transform_power(xd.ptr, ncols, MORLET, F0, 1.0, sj, xh.ptr, Pd.ptr, ld, ncols)
        plan.transform_weighted(xd.ptr, ncols, MORLET, F0, 1.0, sj, xh.ptr, Qd.ptr, ALPHA, Gd.ptr, ld, ncols)
        out = {"W": Wd.download(plan, (rows, ld), cplx), "power": Pd.download(plan, (rows, ld), real),
               "weighted": Gd.download(plan, (rows, ld), cplx)}
    finally:
        for b in bufs:
            b.free()
        plan.close()
    return out, classes, chunks


def assert_same_bits(lib, N, prec, sj, ncols, want=None, min_chunks=1, extra=None):
    old, classes0, chunks0 = outputs(lib, N, prec, sj, ncols, 0, extra=extra)
    new, classes1, chunks1 = outputs(lib, N, prec, sj, ncols, 1, extra=extra)
    assert classes0 == classes1
    assert all(c.startswith("poly/") for c in classes1), classes1       # every row goes through k_poly_rows
    have = {kd_of(c) for c in classes1}
    assert (want or set()) <= have, (sorted(want - have), classes1)
    assert chunks0 == chunks1 and chunks1 >= min_chunks, (chunks0, chunks1)
    for key in ("W", "power", "weighted"):
        a, b = old[key], new[key]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (key, int((a != b).sum()))
        body, pad = b[:, :ncols], b[:, ncols:]
        assert not np.any(body == (SENTINEL if key == "power" else SENTINEL * (1 + 1j))), key     # every column was written
        assert np.all(pad == (SENTINEL if key == "power" else SENTINEL * (1 + 1j))), key          # and no other
    return classes1
