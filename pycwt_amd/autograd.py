"""Differentiable CWT for PyTorch: ``cwt_torch`` runs the transform on torch's current stream (``parallel.HipEngine``) and
its backward through the HIP adjoint of the rows (``cwt_adjoint_rows``): dL/dx = Re(A^H dL/dW) for the real input x, with no
dense filter bank and no activation saved but the geometry of the call."""
import threading

import numpy as np

from . import _hip
from .parallel import HipEngine
from .wavelet import _check_parameter_wavelet, _device_id, _geometry

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
        def forward(ctx, x, eng, kind, param, dt, sj):
            n0 = x.shape[-1]
            cplx_t = torch.complex128 if x.dtype == torch.float64 else torch.complex64
            W = torch.empty(tuple(x.shape[:-1]) + (sj.size, n0), dtype=cplx_t, device=x.device)
            tol = _tolerance()
            _on_current_stream(torch, eng, x.device)
            eng.plan.set_tolerance(tol)
            eng.transform(x, n0, None, kind, param, dt, sj, W, n0)
            ctx.geometry = (eng, kind, param, dt, sj, tol)       # the backward is the transpose of exactly this forward
            return W

        @staticmethod
        @once_differentiable
        def backward(ctx, gW):
            eng, kind, param, dt, sj, tol = ctx.geometry
            real_t = torch.float64 if gW.dtype in (torch.complex128, torch.float64) else torch.float32
            cplx_t = torch.complex128 if real_t == torch.float64 else torch.complex64
            g = gW.to(cplx_t).contiguous()
            rows, n0 = g.shape[-2], g.shape[-1]
            nb = g.shape[0] if g.dim() == 3 else 1
            xbar = torch.empty(tuple(g.shape[:-2]) + (n0,), dtype=real_t, device=g.device)
            _on_current_stream(torch, eng, g.device)
            eng.plan.set_tolerance(tol)
            eng.plan.adjoint_rows(g.data_ptr(), nb, rows * n0, n0, n0, kind, param, dt, sj, xbar.data_ptr(), n0)
            return xbar, None, None, None, None, None

    return CwtRows


_fn = None


def cwt_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, pad=True):
    """Continuous wavelet transform of a torch tensor, differentiable with respect to it.

    x: (n0,) or (B, n0), float64 or float32.  Returns ``(W, sj, freqs, coi)``: W complex128 / complex64 on x's device,
    (rows, n0) or (B, rows, n0), values as ``pycwt_amd.cwt`` gives them (within the accuracy target of
    ``pycwt_amd.set_tolerance`` when that is a number; round-off otherwise); sj, freqs, coi NumPy arrays exactly as
    ``pycwt_amd.cwt`` returns them (Paul's NaN-row rule included).  The backward is the HIP adjoint of the rows on torch's
    current stream.  Built-in mothers and pad=True only.  Tensors must live on a GPU; CPU tensors are accepted only by the
    CPU emulation of the library that the test suite loads."""
    global _fn
    import torch
    if not pad:
        raise ValueError("cwt_torch: pad=False (Bluestein transforms of any length) has no adjoint; use pad=True")
    if not torch.is_tensor(x) or x.dtype not in (torch.float64, torch.float32):
        raise TypeError("cwt_torch: x must be a float64 or float32 torch tensor")
    if x.dim() not in (1, 2) or x.shape[-1] < 1:
        raise ValueError("cwt_torch: x must have shape (n0,) or (B, n0)")
    mother = _check_parameter_wavelet(wavelet)
    if not hasattr(mother, "device_id"):
        raise ValueError("cwt_torch: only the built-in mothers (Morlet, Paul, DOG) have a HIP adjoint")
    lib = _hip.load()
    if x.device.type != "cuda" and lib.backend().startswith("hip"):
        raise RuntimeError("cwt_torch needs a tensor on a GPU (the HIP kernels cannot read host memory)")
    n0 = int(x.shape[-1])
    N, sj, freqs, coi, _, bad = _geometry(mother, n0, dt, dj, s0, J, freqs, True)
    if bad is not None and not bad.all():
        sj, freqs = sj[~bad], np.asarray(freqs)[~bad]
    sj, freqs, coi = np.array(sj, dtype=np.float64), np.array(freqs), np.array(coi)
    kind, param = _device_id(mother)
    nb = int(x.shape[0]) if x.dim() == 2 else 1
    precision = 64 if x.dtype == torch.float64 else 32
    eng = _engine(torch, N, precision, nb * sj.size, x.device, lib)
    if _fn is None:
        _fn = _function(torch)
    W = _fn.apply(x.contiguous(), eng, kind, float(param), float(dt), sj)
    return W, sj, freqs, coi
