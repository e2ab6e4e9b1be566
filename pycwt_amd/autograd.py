"""Differentiable CWT for PyTorch: ``cwt_torch`` runs the transform on torch's current stream (``parallel.HipEngine``) and
its backward through the HIP adjoint of the rows (``cwt_adjoint_rows``): dL/dx = Re(A^H dL/dW) for the real input x, with no
dense filter bank and no activation saved but the geometry of the call.  With ``hop=h`` forward and backward work on every
h-th column only (``cwt_transform_hop``, ``cwt_adjoint_rows_hop``): nothing of rows x n0 elements exists in either."""
import threading

import numpy as np

from . import _hip
from .parallel import HipEngine
from .wavelet import _check_hop, _check_parameter_wavelet, _device_id, _geometry

_engines: dict = {}       # (nfft, precision, device, library) -> HipEngine: keeps the plan and its cached row tables
_engines_lock = threading.Lock()


def _engine(torch, nfft, precision, rows, device, lib):
    key = (nfft, precision, device.type, device.index or 0, id(lib))
    with _engines_lock:
        eng = _engines.get(key)
        if eng is None or eng.plan.max_rows < rows or not eng.plan.h:
            eng = HipEngine(nfft, precision, max(rows, 64), device.index or 0, device.type == "cuda", lib=lib)
            eng.stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None
            _engines[key] = eng
        return eng


def _on_current_stream(torch, eng, device):
    """The plan queues on torch's current stream of `device` (cwt_plan_set_stream synchronises the old one: only on a change)."""
    if device.type != "cuda":
        return
    s = torch.cuda.current_stream(device).cuda_stream
    if s != eng.stream:
        eng.plan.set_stream(s)
        eng.stream = s


def _tolerance():
    """The module's accuracy target (pycwt_amd.set_tolerance) as a fixed tolerance: a float applies as it is; "auto" and None
    run at the engine's round-off default, 0 (the automatic mode reads the spectrum's range back to the host per call)."""
    from . import wavelet
    t = wavelet._tolerance
    return float(t) if isinstance(t, (int, float)) and not isinstance(t, bool) and t else 0.0


def _function(torch):
    from torch.autograd.function import once_differentiable

    class CwtRows(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, eng, kind, param, dt, sj, hop):
            n0 = x.shape[-1]
            cplx_t = torch.complex128 if x.dtype == torch.float64 else torch.complex64
            W = torch.empty(tuple(x.shape[:-1]) + (sj.size, n0 if hop is None else -(-n0 // hop)), dtype=cplx_t, device=x.device)
            tol = _tolerance()
            _on_current_stream(torch, eng, x.device)
            eng.plan.set_tolerance(tol)
            if hop is None:
                eng.transform(x, n0, None, kind, param, dt, sj, W, n0)
            else:
                eng.transform_hop(x, n0, hop, eng.plan.OUT_W, kind, param, dt, sj, W)
            ctx.geometry = (eng, kind, param, dt, sj, tol, hop, n0)   # the backward is the transpose of exactly this forward
            return W

        @staticmethod
        @once_differentiable
        def backward(ctx, gW):
            eng, kind, param, dt, sj, tol, hop, n0 = ctx.geometry
            real_t = torch.float64 if gW.dtype in (torch.complex128, torch.float64) else torch.float32
            cplx_t = torch.complex128 if real_t == torch.float64 else torch.complex64
            g = gW.to(cplx_t).resolve_conj().contiguous()        # (a lazily conjugated cotangent keeps its bits unconjugated in memory)
            rows = g.shape[-2]
            nb = g.shape[0] if g.dim() == 3 else 1
            xbar = torch.empty(tuple(g.shape[:-2]) + (n0,), dtype=real_t, device=g.device)
            _on_current_stream(torch, eng, g.device)
            eng.plan.set_tolerance(tol)
            if hop is None:
                eng.plan.adjoint_rows(g.data_ptr(), nb, rows * n0, n0, n0, kind, param, dt, sj, xbar.data_ptr(), n0)
            else:
                eng.adjoint_rows_hop(g, n0, hop, kind, param, dt, sj, xbar)
            return xbar, None, None, None, None, None, None

    class CwtPower(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, eng, kind, param, dt, sj, hop):
            n0 = x.shape[-1]
            P = torch.empty(tuple(x.shape[:-1]) + (sj.size, n0 if hop is None else -(-n0 // hop)), dtype=x.dtype, device=x.device)
            tol = _tolerance()
            _on_current_stream(torch, eng, x.device)
            eng.plan.set_tolerance(tol)
            if hop is None:
                eng.transform_power(x, n0, None, kind, param, dt, sj, P, n0)
            else:
                eng.transform_hop(x, n0, hop, eng.plan.OUT_POWER, kind, param, dt, sj, P)
            ctx.save_for_backward(x)                             # the signal and the geometry: nothing of rows x n0 elements
            ctx.geometry = (eng, kind, param, dt, sj, tol, hop)
            return P

        @staticmethod
        @once_differentiable
        def backward(ctx, gP):
            (x,) = ctx.saved_tensors
            eng, kind, param, dt, sj, tol, hop = ctx.geometry
            cplx_t = torch.complex128 if x.dtype == torch.float64 else torch.complex64
            q = gP.to(x.dtype).contiguous()
            rows, n0 = q.shape[-2], x.shape[-1]
            nb = q.shape[0] if q.dim() == 3 else 1
            G = torch.empty(q.shape, dtype=cplx_t, device=q.device)
            xbar = torch.empty(tuple(q.shape[:-2]) + (n0,), dtype=x.dtype, device=q.device)
            _on_current_stream(torch, eng, q.device)
            eng.plan.set_tolerance(tol)
            # dL = sum gP 2 Re(conj(W) dW) = Re sum conj(2 gP W) dW: W recomputed from x, weighted in the row kernels' store
            if hop is None:
                eng.transform_weighted(x, n0, None, kind, param, dt, sj, q, 2.0, G, n0)
                eng.plan.adjoint_rows(G.data_ptr(), nb, rows * n0, n0, n0, kind, param, dt, sj, xbar.data_ptr(), n0)
            else:                                                # the same on the kept columns: G is rows x ceil(n0 / hop)
                eng.transform_hop(x, n0, hop, eng.plan.OUT_WEIGHTED, kind, param, dt, sj, G, q, 2.0)
                eng.adjoint_rows_hop(G, n0, hop, kind, param, dt, sj, xbar)
            del G
            return xbar, None, None, None, None, None, None

    return CwtRows, CwtPower


_fn = None


def _prepare(name, x, dt, dj, s0, J, wavelet, freqs, pad, hop=None):
    """The checks, grid and engine of one call of `name` (cwt_torch, cwt_power_torch)."""
    import torch
    if not pad:
        raise ValueError(f"{name}: pad=False (Bluestein transforms of any length) has no adjoint; use pad=True")
    if not torch.is_tensor(x) or x.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"{name}: x must be a float64 or float32 torch tensor")
    if x.dim() not in (1, 2) or x.shape[-1] < 1:
        raise ValueError(f"{name}: x must have shape (n0,) or (B, n0)")
    mother = _check_parameter_wavelet(wavelet)
    if not hasattr(mother, "device_id"):
        raise ValueError(f"{name}: only the built-in mothers (Morlet, Paul, DOG) have a HIP adjoint")
    lib = _hip.load()
    if x.device.type != "cuda" and lib.backend().startswith("hip"):
        raise RuntimeError(f"{name} needs a tensor on a GPU (the HIP kernels cannot read host memory)")
    n0 = int(x.shape[-1])
    N, sj, freqs, coi, _, bad = _geometry(mother, n0, dt, dj, s0, J, freqs, True)
    if bad is not None and not bad.all():
        sj, freqs = sj[~bad], np.asarray(freqs)[~bad]
    sj, freqs, coi = np.array(sj, dtype=np.float64), np.array(freqs), np.array(coi)
    if hop is not None:
        hop = _check_hop(hop, N, mother)
        coi = coi[::hop]
    kind, param = _device_id(mother)
    nb = int(x.shape[0]) if x.dim() == 2 else 1
    precision = 64 if x.dtype == torch.float64 else 32
    eng = _engine(torch, N, precision, nb * sj.size, x.device, lib)
    return torch, eng, kind, float(param), sj, freqs, coi, hop


def cwt_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, pad=True, hop=None):
    """Continuous wavelet transform of a torch tensor, differentiable with respect to it.

    x: (n0,) or (B, n0), float64 or float32.  Returns ``(W, sj, freqs, coi)``: W complex128 / complex64 on x's device,
    (rows, n0) or (B, rows, n0), values as ``pycwt_amd.cwt`` gives them (within the accuracy target of
    ``pycwt_amd.set_tolerance`` when that is a number; round-off otherwise); sj, freqs, coi NumPy arrays exactly as
    ``pycwt_amd.cwt`` returns them (Paul's NaN-row rule included).  The backward is the HIP adjoint of the rows on torch's
    current stream.  Built-in mothers and pad=True only.  Tensors must live on a GPU; CPU tensors are accepted only by the
    CPU emulation of the library that the test suite loads.

    hop=h (a power of two, 16 <= padded length / h <= 4096): W has ceil(n0 / h) columns, equal to columns ``::h`` of the
    undecimated W to rounding, and coi is ``coi[::h]``; the forward computes nothing else (``cwt_transform_hop``) and the
    backward is ``cwt_adjoint_rows_hop`` of the cotangent.  The columns are a SAMPLE of W, not an average over the hop:
    choosing h against the smallest scale is the caller's business."""
    global _fn
    torch, eng, kind, param, sj, freqs, coi, hop = _prepare("cwt_torch", x, dt, dj, s0, J, wavelet, freqs, pad, hop)
    if _fn is None:
        _fn = _function(torch)
    W = _fn[0].apply(x.contiguous(), eng, kind, param, float(dt), sj, hop)
    return W, sj, freqs, coi


def cwt_power_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, pad=True, hop=None):
    """The scalogram ``|W|^2`` of a torch tensor, differentiable with respect to it: ``cwt_torch(x, ...)[0].abs() ** 2`` without
    W -- neither written by the forward nor kept for the backward.

    Inputs, refusals, engine, stream and tolerance as ``cwt_torch``.  Returns ``(P, sj, freqs, coi)``: P float64 / float32 on
    x's device, (rows, n0) or (B, rows, n0), written by the power row kernels (``cwt_transform_power``).  Between forward and
    backward only x and the geometry of the call are held.  The backward recomputes W from x under the cotangent of P in the
    row kernels' store (``cwt_transform_weighted``: G = 2 gP W, complex, freed when the backward returns) and runs the HIP
    adjoint of the rows on G; once differentiable.

    hop=h as in ``cwt_torch``: P has ceil(n0 / h) columns, samples of |W|^2 at columns ``::h`` (not its mean over the hop), coi
    is ``coi[::h]``.  Forward, the transient G of the backward (``cwt_transform_hop`` with the weighted output) and its
    adjoint (``cwt_adjoint_rows_hop``) are all of rows x ceil(n0 / h) elements; x alone is saved."""
    global _fn
    torch, eng, kind, param, sj, freqs, coi, hop = _prepare("cwt_power_torch", x, dt, dj, s0, J, wavelet, freqs, pad, hop)
    if _fn is None:
        _fn = _function(torch)
    P = _fn[1].apply(x.contiguous(), eng, kind, param, float(dt), sj, hop)
    return P, sj, freqs, coi
