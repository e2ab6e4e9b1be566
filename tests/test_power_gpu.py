"""The power output (cwt_transform_power and siblings, cwt_power*) on a real MI355X: at the BASELINE sizes against the complex
output of the same plan (per row max|dP| / max|W|^2 <= 32 eps) and against the oracle (per row max|P - |W_orc|^2| /
max|W_orc|^2 <= 2 tau + tau^2), the batch, the device handle and the canonical NINO3 call."""
import numpy as np
import pytest

import pycwt_amd
from conftest import load_golden
from oracle import cwt_oracle as orc
from pycwt_amd import _hip
from test_power_emulated import EPS32, power_bound

pytestmark = pytest.mark.gpu


def grid(N, rows, mother):
    s0 = 2 / mother.flambda()
    return s0 * 2 ** (np.arange(rows) * np.log2(N / s0) / (rows - 1))


def run(plan, x, kind, param, sj, prec, nb=1):
    """(W, P) of one plan: cwt_transform(_batch) and its power sibling on the same signal(s)"""
    real, cplx = (np.float64, np.complex128) if prec == 64 else (np.float32, np.complex64)
    es = np.dtype(real).itemsize
    N, rows = plan.nfft, len(sj)
    xd, xh = _hip.DeviceBuffer(nb * N * es), _hip.DeviceBuffer(nb * N * 2 * es)
    Wd, Pd = _hip.DeviceBuffer(nb * rows * N * 2 * es), _hip.DeviceBuffer(nb * rows * N * es)
    try:
        xd.upload(plan, np.ascontiguousarray(x, dtype=real))
        if nb == 1:
            plan.transform(xd.ptr, N, kind, param, 1.0, sj, xh.ptr, Wd.ptr, N, N)
            plan.transform_power(xd.ptr, N, kind, param, 1.0, sj, xh.ptr, Pd.ptr, N, N)
        else:
            plan.transform_batch(xd.ptr, nb, N, N, kind, param, 1.0, sj, xh.ptr, Wd.ptr, N, N)
            plan.transform_batch_power(xd.ptr, nb, N, N, kind, param, 1.0, sj, xh.ptr, Pd.ptr, N, N)
        return Wd.download(plan, (nb * rows, N), cplx), Pd.download(plan, (nb * rows, N), real)
    finally:
        for b in (xd, xh, Wd, Pd):
            b.free()


def oracle_bound(P, Wo, tau, W=None):
    """per row max|P - |Wo|^2| / max|Wo|^2 <= 2 tau + tau^2; W given (the complex output of the same plan): tau is at least
    that output's own per-row error against the oracle, which the power inherits"""
    ref = np.abs(Wo) ** 2
    if W is not None:
        tau = max(tau, float((np.abs(W - Wo).max(axis=1) / np.abs(Wo).max(axis=1)).max()))
    err = np.abs(P - ref).max(axis=1) / ref.max(axis=1)
    assert err.max() <= 2 * tau + tau * tau + EPS32[64], (err.max(), tau)


@pytest.mark.parametrize("tau", [None, 1e-9], ids=["roundoff", "bench"])
def test_config2_all_rows(hip_library, tau):
    N = 1 << 20
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, 256, m)
    x = np.random.default_rng(1234).standard_normal(N)
    plan = _hip.Plan(N, 64, max_rows=256, options={} if tau is None else {"tolerance": tau})
    try:
        W, P = run(plan, x, orc.MORLET, 6, sj, 64)
    finally:
        plan.close()
    power_bound(P, W, 64)
    for lo in range(0, 256, 32):                            # the oracle in groups of rows (host memory)
        oracle_bound(P[lo:lo + 32], orc.cwt_rows(x, 1.0, sj[lo:lo + 32], m), 1e-14 if tau is None else tau,
                     W[lo:lo + 32] if tau is None else None)


@pytest.mark.parametrize("kind,param", [(orc.PAUL, 4), (orc.DOG, 2)], ids=["paul", "dog"])
def test_config3_fp32_all_rows(hip_library, kind, param):
    N = 1 << 20
    m = orc.Mother(kind, param)
    sj = grid(N, 256, m)
    sj = sj[~orc.dropped_rows(sj, 1.0, m)]
    x = np.random.default_rng(1234).standard_normal(N).astype(np.float32)
    plan = _hip.Plan(N, 32, max_rows=256, options={"tolerance": 3e-5})
    try:
        W, P = run(plan, x, kind, param, sj, 32)
    finally:
        plan.close()
    power_bound(P, W, 32)


def test_config4_batch_sampled(hip_library):
    N, nb, rows = 1 << 16, 16, 128
    m = orc.Mother(orc.MORLET, 6)
    sj = grid(N, rows, m)
    X = np.random.default_rng(5).standard_normal((nb, N))
    plan = _hip.Plan(N, 64, max_rows=nb * rows, options={"tolerance": 1e-9})
    try:
        W, P = run(plan, X, orc.MORLET, 6, sj, 64, nb=nb)
    finally:
        plan.close()
    power_bound(P, W, 64)
    rng = np.random.default_rng(6)
    for b in rng.choice(nb, 3, replace=False):
        js = np.sort(rng.choice(rows, 6, replace=False))
        oracle_bound(P[b * rows + js], orc.cwt_rows(X[b], 1.0, sj[js], m), 1e-9)


def test_device_handle_reductions(hip_library):
    x = np.random.default_rng(7).standard_normal(1 << 18)
    h = pycwt_amd.cwt_power_device(x, 1.0, 1 / 8)
    try:
        P = h.power()
        power_bound(P, pycwt_amd.cwt(x, 1.0, 1 / 8)[0], 64)
        np.testing.assert_allclose(h.global_power(), P.mean(axis=1), rtol=1e-12)
        w = np.where((h.sj >= 4.0) & (h.sj < 64.0), 1.0 / h.sj, 0.0)
        np.testing.assert_allclose(h.scale_average(4.0, 64.0, 1 / 8), (1 / 8) / h.mother.cdelta * (w[:, None] * P).sum(axis=0),
                                   rtol=1e-12)
    finally:
        h.close()


def test_nino3_canonical_call(hip_library):
    g = load_golden("nino3_default")
    out = pycwt_amd.cwt_power(g["x"], 0.25, wavelet="morlet")
    ref = np.abs(g["W"]) ** 2
    assert out[0].shape == ref.shape and out[0].dtype == np.float64
    assert (np.abs(out[0] - ref).max(axis=1) / ref.max(axis=1)).max() <= 1e-10     # 2 x the W bound of test_gpu_parity
    W = pycwt_amd.cwt(g["x"], 0.25, wavelet="morlet")
    power_bound(out[0], W[0], 64)
    for a, b in zip(out[1:], W[1:]):
        assert np.array_equal(a, b)
