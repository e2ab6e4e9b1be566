"""The plan calls of pycwt_amd.autograd, case by case, on the CPU emulation of the HIP runtime (tests/emu): every device action
of the torch layer is one method of `_hip.Plan`, so the sequence of those calls with their integer and floating-point arguments
IS what a forward or a backward does on the device.  Each case's forward and backward are recorded separately and compared with
a literal list; beside the sequence, what each node holds between the two (`saved_tensors`, the geometry).  A backward that
returns another number of values than its forward took raises in autograd: a backward that completes is that check.

A record is a list of (method, arguments): the arguments that are not device addresses, in the method's own order -- integers,
floats (12 significant digits), booleans and None as they are, arrays (the scales, the weights, the ranks) as their length; an
address appears only where it is None (an output that was not asked for).  A `set_tolerance` that repeats the value already in
force in the record is dropped: it stores one field.

`make_cases` builds the cases for any module with the interface of pycwt_amd.autograd and any length, for scripts that compare
two implementations bit by bit.
"""
import inspect
import numbers

import numpy as np
import pytest

import pycwt_amd
from pycwt_amd import _hip

torch = pytest.importorskip("torch")

N0, HOP, POOL = 100, 4, 4                  # padded to 128; x (100,) and (2, 100); dt = 1, dj = 1 / 2, float64
SCALES = [2.0, 4.0, 8.0]
PAUL_SCALES = [2.0, 300.0, 8.0]            # Paul's NaN-row rule drops s > 709 / pi at dt = 1: the mask of kept scales has a hole


class Recorder:
    """Every public method of _hip.Plan appends (name, arguments) to `calls` while a record is open."""

    def __init__(self, monkeypatch):
        self.calls = None
        for name, fn in list(vars(_hip.Plan).items()):
            if name.startswith("_") or name == "close" or not inspect.isfunction(fn):
                continue
            monkeypatch.setattr(_hip.Plan, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def wrapper(plan, *a, **kw):
            if self.calls is not None:
                bound = sig.bind(plan, *a, **kw)
                bound.apply_defaults()
                self.calls.append((name, tuple(self._values(list(bound.arguments.items())[1:]))))
            return fn(plan, *a, **kw)
        return wrapper

    @staticmethod
    def _values(items):
        for key, v in items:
            address = key.endswith("_dev") or key == "stream_handle"
            if v is None:
                yield None
            elif address:
                continue
            elif isinstance(v, (bool, np.bool_)):
                yield bool(v)
            elif isinstance(v, numbers.Integral):
                yield int(v)
            elif isinstance(v, numbers.Real):
                yield float("%.12g" % v)
            elif isinstance(v, (np.ndarray, list, tuple)):
                yield len(v)
            elif isinstance(v, str):
                yield v

    def record(self, fn):
        """(what fn returns, the calls it made)"""
        self.calls = []
        try:
            out = fn()
        finally:
            calls, self.calls = self.calls, None
        kept, tol = [], None
        for name, args in calls:
            if name == "set_tolerance":
                if args == tol:
                    continue
                tol = args
            kept.append((name, args))
        return out, kept


@pytest.fixture()
def recorded(emulated, monkeypatch):
    """pycwt_amd.autograd on the emulated library with an engine cache of the test's own, and the recorder"""
    from pycwt_amd import autograd
    monkeypatch.setattr(autograd, "_engines", {})
    yield autograd, Recorder(monkeypatch)
    for eng in autograd._engines.values():
        eng.plan.close()


def make_cases(api, n0=N0, hop=HOP, pool=POOL, device="cpu"):
    """name -> (run, kind, what the node saves): run() calls `api` on fresh leaves and returns (the outputs, the first of which
    the test differentiates through abs().sum(); the leaves by name).  Signals on `device`, scales and f0 on the CPU."""
    rng = np.random.default_rng(2026)
    X1, X2 = rng.standard_normal(n0), rng.standard_normal((2, n0))
    XN = X2.copy()
    XN[1, n0 // 3] = np.nan
    grid = pycwt_amd.wavelet._geometry(pycwt_amd.Morlet(6), n0, 1.0, 1 / 2, -1, -1, None, True)[1]      # the scales of dj = 1 / 2
    WN = rng.standard_normal((2, len(SCALES), n0)) + 1j * rng.standard_normal((2, len(SCALES), n0))
    sj = np.array(SCALES)

    def leaf(a, grad=True, dev=device):
        return torch.tensor(a, device=dev).requires_grad_(grad)

    def cwt_case(power, X, x_grad=True, scales=None, scales_grad=False, f0=False, wavelet="morlet", **kw):
        def run():
            leaves, extra = {}, {}
            x = leaf(X, x_grad)
            if x_grad:
                leaves["x"] = x
            if scales is not None:
                extra["scales"] = leaf(np.asarray(scales, dtype=np.float64), scales_grad, "cpu")
                if scales_grad:
                    leaves["scales"] = extra["scales"]
            if f0:
                extra["f0"] = leaves["f0"] = leaf(np.float64(6.0), True, "cpu")
            fn = api.cwt_power_torch if power else api.cwt_torch
            grid_kw = {} if scales is not None else {"dj": 1 / 2}
            return (fn(x, 1.0, wavelet=wavelet, **grid_kw, **kw, **extra)[0],), leaves
        return run, "power" if power else "cwt", "x" if power or scales is not None or f0 else "nothing"

    cases = {}
    for shape, X in (("single", X1), ("batch", X2)):
        cases[f"cwt-{shape}"] = cwt_case(False, X)
        cases[f"cwt-hop-{shape}"] = cwt_case(False, X, hop=hop)
        cases[f"power-{shape}"] = cwt_case(True, X)
        cases[f"power-hop-{shape}"] = cwt_case(True, X, hop=hop)
        cases[f"power-pool-{shape}"] = cwt_case(True, X, pool=pool)
    cases["cwt-scales-const"] = cwt_case(False, X1, scales=grid)
    cases["cwt-scales-grad"] = cwt_case(False, X1, scales=SCALES, scales_grad=True)
    cases["cwt-scales-f0-grad-hop"] = cwt_case(False, X2, scales=SCALES, scales_grad=True, f0=True, hop=hop)
    cases["cwt-scales-grad-x-const"] = cwt_case(False, X2, x_grad=False, scales=SCALES, scales_grad=True)
    cases["cwt-paul-dropped-scale"] = cwt_case(False, X1, scales=PAUL_SCALES, scales_grad=True, wavelet=pycwt_amd.Paul(4))
    cases["power-hop-scales-grad"] = cwt_case(True, X1, scales=SCALES, scales_grad=True, hop=hop)
    cases["power-pool-scales-f0-grad"] = cwt_case(True, X2, scales=SCALES, scales_grad=True, f0=True, pool=pool)

    def ssq():
        x = leaf(XN)
        return (api.ssq_cwt_torch(x, 1.0, 1 / 2, gamma=1e-8)[0],), {"x": x}

    def icwt():
        W = leaf(WN[0])
        return (api.icwt_torch(W, sj, 1.0, 1 / 2),), {"W": W}

    def shrink():
        W, lam = leaf(WN), leaf(np.array([0.5, 1.0, 1.5]))
        return (api.icwt_shrink_torch(W, sj, 1.0, lam, 1 / 2, mode="soft"),), {"W": W, "lam": lam}

    def denoise_universal():
        x, scale = leaf(XN), leaf(np.float64(1.0), True, "cpu")
        y, lam = api.denoise_torch(x, 1.0, 1 / 2, scale=scale)[:2]
        return (y, lam), {"x": x, "scale": scale}

    def denoise_tensor():
        x, lam = leaf(XN), leaf(np.full(grid.size, 0.7))
        y, used = api.denoise_torch(x, 1.0, 1 / 2, threshold=lam)[:2]
        return (y, used), {"x": x, "lam": lam}

    cases["ssq-batch-nan"] = ssq, "ssq", None
    cases["icwt"] = icwt, "icwt", None
    cases["icwt-shrink-soft"] = shrink, "shrink", None
    cases["denoise-universal-batch-nan"] = denoise_universal, "denoise", None
    cases["denoise-tensor-batch-nan"] = denoise_tensor, "denoise", None
    return cases


# kind: Morlet 0, Paul 1; the arguments in the order of the methods of _hip.Plan (see Recorder._values)
TOL = ("set_tolerance", (0.0,))
ADJ1 = ("adjoint_rows", (1, 1200, 100, 100, 0, 6.0, 1.0, 12, 100, False))          # one signal's 12 rows x 100 columns
W1 = ("transform", (100, 0, 6.0, 1.0, 12, None, 100, 100))                         # (None: no spectrum asked for)
EXPECTED = {                               # name: (forward, backward)
    "cwt-single": ([TOL, W1], [TOL, ADJ1]),
    "cwt-batch": (
        [TOL, ("transform_batch", (2, 100, 100, 0, 6.0, 1.0, 12, 100, 100))],
        [TOL, ("adjoint_rows", (2, 1200, 100, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "cwt-hop-single": (
        [TOL, ("transform_hop", (1, 100, 100, 0, 6.0, 1.0, 12, 4, None, 0, 25, None, 0.0))],
        [TOL, ("adjoint_rows_hop", (1, 300, 25, 4, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "cwt-hop-batch": (
        [TOL, ("transform_hop", (2, 100, 100, 0, 6.0, 1.0, 12, 4, None, 0, 25, None, 0.0))],
        [TOL, ("adjoint_rows_hop", (2, 300, 25, 4, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "cwt-scales-const": ([TOL, W1], [TOL, ADJ1]),
    "cwt-scales-grad": (
        [TOL, ("transform", (100, 0, 6.0, 1.0, 3, None, 100, 100))],
        [TOL, ("fft_rows", (False, 1, 100, 100)),
         ("adjoint_rows_scales", (1, 300, 100, None, 100, 128, 0, 6.0, 1.0, 3, 100, False))]),
    "cwt-scales-f0-grad-hop": (
        [TOL, ("transform_hop", (2, 100, 100, 0, 6.0, 1.0, 3, 4, None, 0, 25, None, 0.0))],
        [TOL, ("fft_rows", (False, 2, 100, 100)),
         ("adjoint_rows_scales", (2, 75, 25, 4, 100, 128, 0, 6.0, 1.0, 3, 100, False))]),
    "cwt-scales-grad-x-const": (
        [TOL, ("transform_batch", (2, 100, 100, 0, 6.0, 1.0, 3, 100, 100))],
        [TOL, ("fft_rows", (False, 2, 100, 100)),
         ("adjoint_rows_scales", (2, 300, 100, None, 100, 128, 0, 6.0, 1.0, 3, None, 100, False))]),
    "cwt-paul-dropped-scale": (
        [TOL, ("transform", (100, 1, 4.0, 1.0, 2, None, 100, 100))],
        [TOL, ("fft_rows", (False, 1, 100, 100)),
         ("adjoint_rows_scales", (1, 200, 100, None, 100, 128, 1, 4.0, 1.0, 2, 100, False))]),
    "power-single": (
        [TOL, ("transform_power", (100, 0, 6.0, 1.0, 12, None, 100, 100))],
        [TOL, ("transform_weighted", (100, 0, 6.0, 1.0, 12, None, 2.0, 100, 100)), ADJ1]),
    "power-batch": (
        [TOL, ("transform_batch_power", (2, 100, 100, 0, 6.0, 1.0, 12, 100, 100))],
        [TOL, ("transform_batch_weighted", (2, 100, 100, 0, 6.0, 1.0, 12, 2.0, 100, 100)),
         ("adjoint_rows", (2, 1200, 100, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "power-hop-single": (
        [TOL, ("transform_hop", (1, 100, 100, 0, 6.0, 1.0, 12, 4, None, 1, 25, None, 0.0))],
        [TOL, ("transform_hop", (1, 100, 100, 0, 6.0, 1.0, 12, 4, None, 2, 25, 2.0)),
         ("adjoint_rows_hop", (1, 300, 25, 4, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "power-hop-batch": (
        [TOL, ("transform_hop", (2, 100, 100, 0, 6.0, 1.0, 12, 4, None, 1, 25, None, 0.0))],
        [TOL, ("transform_hop", (2, 100, 100, 0, 6.0, 1.0, 12, 4, None, 2, 25, 2.0)),
         ("adjoint_rows_hop", (2, 300, 25, 4, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "power-pool-single": (
        [TOL, ("transform_pool", (1, 100, 100, 0, 6.0, 1.0, 12, 4, None, 25))],
        [TOL, ("transform_weighted", (100, 0, 6.0, 1.0, 12, None, 2.0, 100, 100)), ADJ1]),
    "power-pool-batch": (
        [TOL, ("transform_pool", (2, 100, 100, 0, 6.0, 1.0, 12, 4, None, 25))],
        [TOL, ("transform_batch_weighted", (2, 100, 100, 0, 6.0, 1.0, 12, 2.0, 100, 100)),
         ("adjoint_rows", (2, 1200, 100, 100, 0, 6.0, 1.0, 12, 100, False))]),
    "power-hop-scales-grad": (
        [TOL, ("transform_hop", (1, 100, 100, 0, 6.0, 1.0, 3, 4, None, 1, 25, None, 0.0))],
        [TOL, ("transform_hop", (1, 100, 100, 0, 6.0, 1.0, 3, 4, None, 2, 25, 2.0)), ("fft_rows", (False, 1, 100, 100)),
         ("adjoint_rows_scales", (1, 75, 25, 4, 100, 128, 0, 6.0, 1.0, 3, 100, False))]),
    "power-pool-scales-f0-grad": (
        [TOL, ("transform_pool", (2, 100, 100, 0, 6.0, 1.0, 3, 4, None, 25))],
        [TOL, ("transform_batch_weighted", (2, 100, 100, 0, 6.0, 1.0, 3, 2.0, 100, 100)), ("fft_rows", (False, 2, 100, 100)),
         ("adjoint_rows_scales", (2, 300, 100, None, 100, 128, 0, 6.0, 1.0, 3, 100, False))]),
    "ssq-batch-nan": (                     # the calls of the first signal alone
        [TOL, ("transform", (100, 0, 6.0, 1.0, 12, 100, 100)), ("spectrum_derivative", (1.0,)),
         ("transform_rows", (0, 6.0, 1.0, 12, 100, 100)),
         ("ssq_reassign_bins", (100, 100, 12, 1e-08, 0.011048543456, 0.5, 12, 100, False, 100))],
        [TOL, ("ssq_gather", (100, 12, 100, 12, 100, 100)), ADJ1]),
    "icwt": (
        [("icwt_reduce", (100, 100, 3, 1.0))],
        [("icwt_shrink_adjoint", (100, 100, 3, None, 0, 1.0, 100, None, False))]),
    "icwt-shrink-soft": (                  # a batch of 2
        [("icwt_shrink", (100, 100, 3, "soft", 1.0))] * 2,
        [("icwt_shrink_adjoint", (100, 100, 3, "soft", 1.0, 100, False))] * 2),
    "denoise-universal-batch-nan": (       # the calls of the first signal alone; the median of 100 columns is two ranks
        [TOL, W1, ("row_order_statistics", (True, 100, 100, 12, 2, 8)), ("icwt_shrink", (100, 100, 12, "soft", 1.0))],
        [TOL, W1, ("icwt_shrink_adjoint", (100, 100, 12, "soft", 1.0, 100, False)), ADJ1]),
    "denoise-tensor-batch-nan": (
        [TOL, W1, ("icwt_shrink", (100, 100, 12, "soft", 1.0))],
        [TOL, W1, ("icwt_shrink_adjoint", (100, 100, 12, "soft", 1.0, 100, False)), ADJ1]),
}


def held_by(node):
    g = node.geometry
    return tuple(g) if isinstance(g, tuple) else tuple(vars(g).values())


@pytest.mark.parametrize("name", list(EXPECTED))
def test_plan_calls_and_what_the_node_holds(recorded, name):
    autograd, rec = recorded
    cases = make_cases(autograd)
    assert set(cases) == set(EXPECTED)
    run, kind, saves = cases[name]
    (outs, leaves), forward = rec.record(run)
    out = outs[0]
    print(name, "forward ", forward)
    if saves == "nothing":            # cwt_torch without scales= / f0=: no activation saved but the geometry, and no tensor in that
        assert out.grad_fn.saved_tensors == ()
        assert not any(torch.is_tensor(v) for v in held_by(out.grad_fn))
    elif saves == "x":                # with scales= or f0=, and the scalogram in every variant: x alone
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 1 and saved[0].shape[-1] == N0 and saved[0].dtype == torch.float64 and not saved[0].is_complex()
    _, backward = rec.record(lambda: out.abs().sum().backward())
    print(name, "backward", backward)
    for key, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, key
    assert (forward, backward) == EXPECTED[name]

    called = [c[0] for c in forward + backward]
    if name == "cwt-scales-const":                # scales= without a gradient: the backward of the call without the keyword
        assert backward == EXPECTED["cwt-single"][1]
    if kind in ("cwt", "power") and "scales" not in leaves and "f0" not in leaves:
        assert "fft_rows" not in called and "adjoint_rows_scales" not in called
    if name == "cwt-paul-dropped-scale":
        g = leaves["scales"].grad.numpy()
        assert out.shape == (2, N0) and g[1] == 0 and g[0] != 0 and g[2] != 0
    if name == "cwt-scales-grad-x-const":         # xbar is neither allocated nor computed: the address handed over is None
        assert [a for c, a in backward if c == "adjoint_rows_scales"][0].count(None) == 2       # hop and xbar
    if name == "ssq-batch-nan":                   # the signal with the NaN: no plan call in either direction
        assert called.count("transform") == 1 and called.count("adjoint_rows") == 1 and called.count("ssq_gather") == 1
        assert torch.isnan(out[1]).all() and torch.isnan(leaves["x"].grad[1]).all() and torch.isfinite(leaves["x"].grad[0]).all()
    if kind == "denoise":
        assert called.count("transform") == 2 and called.count("adjoint_rows") == 1
    if kind in ("icwt", "shrink"):                # the inverse sets no tolerance
        assert "set_tolerance" not in called
