"""Differentiable CWT for PyTorch: ``cwt_torch`` runs the transform on torch's current stream (``parallel.HipEngine``) and
its backward through the HIP adjoint of the rows (``cwt_adjoint_rows``): dL/dx = Re(A^H dL/dW) for the real input x, with no
dense filter bank and no activation saved but the geometry of the call.  With ``hop=h`` forward and backward work on every
h-th column only (``cwt_transform_hop``, ``cwt_adjoint_rows_hop``): nothing of rows x n0 elements exists in either.  With
``scales=`` (a torch tensor) and, for Morlet, ``f0=`` the transform is differentiable in those too (``cwt_adjoint_rows_scales``:
one reduction over each row's band on the spectra the adjoint forms anyway).  The way back out of the wavelet domain is
``icwt_torch`` / ``icwt_shrink_torch`` / ``denoise_torch``: the (thresholded) inverse and its HIP adjoint
(``cwt_icwt_shrink_adjoint``), differentiable in W, in the thresholds and, for ``denoise_torch``, in x without a saved W."""
import functools
import threading
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _hip
from . import wavelet as _wavelet
from .parallel import HipEngine
from .wavelet import (_band_weights, _check_hop, _check_pool, _pool_coi, _check_parameter_wavelet, _coi, _device_id, _geometry, _nan_rows,
                      _next_pow2, _ssq_grid, _ssq_mother)

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
    t = _wavelet._tolerance
    return float(t) if isinstance(t, (int, float)) and not isinstance(t, bool) and t else 0.0


def _begin(torch, eng, device, tol):
    """What every forward and backward of a transform starts with: the plan on torch's current stream, at this tolerance."""
    _on_current_stream(torch, eng, device)
    eng.plan.set_tolerance(tol)


def _real_of(torch, dtype):
    return torch.float64 if dtype in (torch.complex128, torch.float64) else torch.float32


def _complex_of(torch, dtype):
    return torch.complex128 if dtype in (torch.complex128, torch.float64) else torch.complex64


# what a node of CwtRows / CwtPower holds of its call: the backward is the transpose of exactly this forward
_Geometry = namedtuple("_Geometry", "eng kind param dt sj tol hop pool n0 keep scales f0")


@functools.lru_cache(maxsize=None)
def _functions():
    """The autograd Functions by name, built on first use (importing this module does not import torch)."""
    import torch
    from torch.autograd.function import once_differentiable
    OUT_W, OUT_POWER, OUT_WEIGHTED = _hip.Plan.OUT_W, _hip.Plan.OUT_POWER, _hip.Plan.OUT_WEIGHTED

    def output_columns(g):
        return g.n0 if g.hop is None and g.pool is None else -(-g.n0 // (g.pool if g.pool is not None else g.hop))

    def run_forward(g, x, out, output, Q=None, alpha=0.0):
        """The one engine call that transforms x into `out` under the geometry g: W, |W|^2 (its window means with g.pool) or
        (alpha Q) W.  With g.hop on the kept columns; the weighted output is at the full rate whatever g.pool."""
        n0 = x.shape[-1]
        if g.hop is not None:
            g.eng.transform_hop(x, n0, g.hop, output, g.kind, g.param, g.dt, g.sj, out, Q, alpha)
        elif output == OUT_W:
            g.eng.transform(x, n0, None, g.kind, g.param, g.dt, g.sj, out, n0)
        elif output == OUT_WEIGHTED:
            g.eng.transform_weighted(x, n0, None, g.kind, g.param, g.dt, g.sj, Q, alpha, out, n0)
        elif g.pool is not None:
            g.eng.transform_pool(x, n0, g.pool, g.kind, g.param, g.dt, g.sj, out)
        else:
            g.eng.transform_power(x, n0, None, g.kind, g.param, g.dt, g.sj, out, n0)

    def run_adjoint(g, G, xbar):
        """xbar = Re A^H G for the cotangent G of W under the geometry g (on the kept columns with g.hop)"""
        if g.hop is None:
            g.eng.adjoint_rows(G, g.n0, g.kind, g.param, g.dt, g.sj, xbar)
        else:
            g.eng.adjoint_rows_hop(G, g.n0, g.hop, g.kind, g.param, g.dt, g.sj, xbar)

    def spread_over_windows(q, n0, pool):
        """gP (..., rows, ceil(n0 / pool)) -> (..., rows, n0): gP[j, n // pool] / c_m, c_m the columns of window m inside n0"""
        ncols = q.shape[-1]
        count = torch.full((ncols,), float(pool), dtype=q.dtype, device=q.device)
        count[-1] = float(n0 - (ncols - 1) * pool)
        return (q / count).repeat_interleave(pool, dim=-1)[..., :n0].contiguous()

    def rows_backward(ctx, G):
        """What CwtRows and CwtPower do with the cotangent G of W (complex, contiguous), the plan set up by the caller:
        (xbar, grad_scales, grad_f0), None where no gradient is asked.  Without a scale or f0 gradient that is the adjoint of the
        rows alone, and the saved x is not looked at."""
        g = ctx.geometry
        need_x, need_s, need_f = ctx.needs_input_grad[:3]
        learn = need_s or need_f
        xbar = None
        if need_x or not learn:
            xbar = torch.empty(tuple(G.shape[:-2]) + (g.n0,), dtype=_real_of(torch, G.dtype), device=G.device)
        if not learn:
            run_adjoint(g, G, xbar)
            return xbar, None, None
        (x,) = ctx.saved_tensors
        xs = x if x.dim() == 2 else x[None]
        xhat = g.eng._spectra(xs, G)                            # the signals' spectra, recomputed: x alone was saved
        g.eng.forward(xs, g.n0, xhat)
        sgrad = torch.empty((G.shape[-2], 2), dtype=torch.float64, device=G.device)
        g.eng.adjoint_rows_scales(G, g.n0, g.hop, xhat, g.kind, g.param, g.dt, g.sj, xbar, sgrad)
        gs = gf = None
        if need_s:                                              # d/ds = (d/d ln s) / s; the rows Paul's NaN rule dropped get 0
            part = sgrad[:, 0] / torch.as_tensor(g.sj, dtype=torch.float64, device=sgrad.device)
            gs = torch.zeros(g.scales.shape, dtype=torch.float64, device=sgrad.device)
            gs[torch.as_tensor(g.keep, device=sgrad.device)] = part
            gs = gs.to(g.scales.device)
        if need_f:
            gf = sgrad[:, 1].sum().to(g.f0.device)
        return xbar, gs, gf

    class CwtRows(torch.autograd.Function):
        """W of x.  `scales` and `f0` (None where the caller gave none) are differentiable inputs whose values reach the kernels
        through `sj` and `param`; only with one of them is x saved."""
        @staticmethod
        def forward(ctx, x, scales, f0, eng, kind, param, dt, sj, hop, keep):
            g = _Geometry(eng, kind, param, dt, sj, _tolerance(), hop, None, x.shape[-1], keep, scales, f0)
            W = torch.empty(tuple(x.shape[:-1]) + (sj.size, output_columns(g)), dtype=_complex_of(torch, x.dtype), device=x.device)
            _begin(torch, eng, x.device, g.tol)
            run_forward(g, x, W, OUT_W)
            if scales is not None or f0 is not None:
                ctx.save_for_backward(x)
            ctx.geometry = g
            return W

        @staticmethod
        @once_differentiable
        def backward(ctx, gW):
            g = ctx.geometry
            # (a lazily conjugated cotangent keeps its bits unconjugated in memory)
            G = gW.to(_complex_of(torch, gW.dtype)).resolve_conj().contiguous()
            _begin(torch, g.eng, G.device, g.tol)
            return rows_backward(ctx, G) + (None,) * 7

    class CwtPower(torch.autograd.Function):
        """|W|^2 of x (its window means with `pool`), `scales` and `f0` as in CwtRows.  Saved: the signal and the geometry,
        nothing of rows x n0 elements."""
        @staticmethod
        def forward(ctx, x, scales, f0, eng, kind, param, dt, sj, hop, keep, pool):
            g = _Geometry(eng, kind, param, dt, sj, _tolerance(), hop, pool, x.shape[-1], keep, scales, f0)
            P = torch.empty(tuple(x.shape[:-1]) + (sj.size, output_columns(g)), dtype=x.dtype, device=x.device)
            _begin(torch, eng, x.device, g.tol)
            run_forward(g, x, P, OUT_POWER)
            ctx.save_for_backward(x)
            ctx.geometry = g
            return P

        @staticmethod
        @once_differentiable
        def backward(ctx, gP):
            (x,) = ctx.saved_tensors
            g = ctx.geometry
            q = gP.to(x.dtype).contiguous()
            if g.pool is not None:                               # the cotangent of |W|^2 at the full rate: gP / c_m on every column of window m
                q = spread_over_windows(q, g.n0, g.pool)
            G = torch.empty(q.shape, dtype=_complex_of(torch, x.dtype), device=q.device)
            _begin(torch, g.eng, q.device, g.tol)
            # dL = sum gP 2 Re(conj(W) dW) = Re sum conj(2 gP W) dW: W recomputed from x, weighted in the row kernels' store
            # (with hop on the kept columns: G is rows x ceil(n0 / hop))
            run_forward(g, x, G, OUT_WEIGHTED, q, 2.0)
            out = rows_backward(ctx, G)
            del G
            return out + (None,) * 8

    class SsqRows(torch.autograd.Function):
        """The synchrosqueezed transform of x (n0,) or (B, n0), signal by signal.  Between forward and backward only the map of
        bins (int16, ... x rows x n0) and the geometry are held: neither x, W nor dW."""
        @staticmethod
        def forward(ctx, x, eng, kind, param, dt, sj, grid, gammas):
            f_lo, dv, nf = grid
            n0, rows = x.shape[-1], sj.size
            cplx_t = _complex_of(torch, x.dtype)
            Tx = torch.empty(tuple(x.shape[:-1]) + (nf, n0), dtype=cplx_t, device=x.device)
            bins = torch.empty(tuple(x.shape[:-1]) + (rows, n0), dtype=torch.int16, device=x.device)
            tol = _tolerance()
            _begin(torch, eng, x.device, tol)
            es = 8 if x.dtype == torch.float64 else 4
            chunk = _wavelet.SSQ_CHUNK_ROWS or max(1, _wavelet._pool_limit(eng.plan.lib, x.device.index or 0) // (n0 * 2 * es))
            chunk = int(min(rows, chunk))
            w = 1.0 / np.sqrt(sj)
            W = torch.empty((rows, n0), dtype=cplx_t, device=x.device)
            dW = torch.empty((chunk, n0), dtype=cplx_t, device=x.device)
            xhat = torch.empty((eng.plan.nfft,), dtype=cplx_t, device=x.device)
            for xb, Tb, bb, gamma in zip(x.reshape(-1, n0), Tx.reshape(-1, nf, n0), bins.reshape(-1, rows, n0), gammas):
                if gamma is None:                                # a non-finite sample: every element of W is NaN, so is every cell of T
                    Tb.fill_(complex(float("nan"), float("nan")))
                    bb.fill_(-1)
                    continue
                eng.transform(xb, n0, xhat, kind, param, dt, sj, W, n0)                    # W as CwtRows.forward computes it
                eng.plan.spectrum_derivative(xhat.data_ptr(), dt, xhat.data_ptr())        # the spectrum times i w, in place
                for a in range(0, rows, chunk):
                    b = min(rows, a + chunk)
                    eng.rows(xhat, kind, param, dt, sj[a:b], dW[:b - a], n0)
                    eng.ssq_reassign_bins(W[a:b], dW[:b - a], w[a:b], gamma, f_lo, dv, Tb, a > 0, bb[a:b])
            del W, dW, xhat
            ctx.save_for_backward(bins)
            ctx.geometry = (eng, kind, param, dt, sj, tol, nf, n0, [g is not None for g in gammas])
            ctx.ssq_map = True                                   # (what _ssq_saved_bins recognises the node by)
            return Tx

        @staticmethod
        @once_differentiable
        def backward(ctx, gT):
            (bins,) = ctx.saved_tensors
            eng, kind, param, dt, sj, tol, nf, n0, finite = ctx.geometry
            cplx_t = _complex_of(torch, gT.dtype)
            g = gT.to(cplx_t).resolve_conj().contiguous()        # (a lazily conjugated cotangent keeps its bits unconjugated in memory)
            rows = sj.size
            xbar = torch.empty(tuple(g.shape[:-2]) + (n0,), dtype=_real_of(torch, gT.dtype), device=g.device)
            _begin(torch, eng, g.device, tol)
            w = 1.0 / np.sqrt(sj)
            G = torch.empty((rows, n0), dtype=cplx_t, device=g.device)      # one signal's rows x n0, whatever the batch
            for gb, bb, xb, ok in zip(g.reshape(-1, nf, n0), bins.reshape(-1, rows, n0), xbar.reshape(-1, n0), finite):
                if not ok:
                    xb.fill_(float("nan"))
                    continue
                eng.ssq_gather(gb, bb, w, G)
                eng.adjoint_rows(G, n0, kind, param, dt, sj, xb)
            del G
            return xbar, None, None, None, None, None, None, None

    def shrink_inverse(eng, Wb, sj, lam_b, mode, out_b):
        """out_b = sum_j Re eta(W[j]; lam[j]) / sqrt(s_j) of one signal (lam_b None: the plain inverse), coeff = 1"""
        n0 = Wb.shape[-1]
        if lam_b is None:
            eng.plan.icwt_reduce(Wb.data_ptr(), n0, n0, sj, 1.0, out_b.data_ptr())
        else:
            eng.plan.icwt_shrink(Wb.data_ptr(), n0, n0, sj, lam_b.data_ptr(), mode, 1.0, out_b.data_ptr())

    class IcwtShrink(torch.autograd.Function):
        """sum_j Re eta(W[j, n]; lam_j) / sqrt(s_j) of W (B, rows, n0) and lam (B, rows) of W's precision, or None (the plain
        inverse), signal by signal.  Saves W and lam; the backward is cwt_icwt_shrink_adjoint."""
        @staticmethod
        def forward(ctx, W, lam, eng, sj, mode):
            out = torch.empty((W.shape[0], W.shape[-1]), dtype=_real_of(torch, W.dtype), device=W.device)
            _on_current_stream(torch, eng, W.device)
            for b in range(W.shape[0]):
                shrink_inverse(eng, W[b], sj, None if lam is None else lam[b], mode, out[b])
            if lam is None:
                ctx.shape = (tuple(W.shape), W.dtype, W.device)
            else:
                ctx.save_for_backward(W, lam)
            ctx.geometry = (eng, sj, mode)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gy):
            eng, sj, mode = ctx.geometry
            if ctx.saved_tensors:
                W, lam = ctx.saved_tensors
                shape, dtype, device = tuple(W.shape), W.dtype, W.device
            else:
                W, lam = None, None
                shape, dtype, device = ctx.shape
            g = gy.to(_real_of(torch, dtype)).contiguous()
            n0 = shape[-1]
            G = torch.empty(shape, dtype=dtype, device=device)
            glam = None if lam is None else torch.empty(lam.shape, dtype=torch.float64, device=device)
            _on_current_stream(torch, eng, device)
            for b in range(shape[0]):
                if lam is None:                                  # (W is not read: G stands in for the pointer)
                    eng.plan.icwt_shrink_adjoint(G[b].data_ptr(), n0, n0, sj, None, 0, 1.0, g[b].data_ptr(), G[b].data_ptr(), n0)
                else:
                    eng.plan.icwt_shrink_adjoint(W[b].data_ptr(), n0, n0, sj, lam[b].data_ptr(), mode, 1.0, g[b].data_ptr(),
                                                 G[b].data_ptr(), n0, glam[b].data_ptr())
            return G, None if lam is None else glam.to(lam.dtype), None, None, None

    class DenoiseRows(torch.autograd.Function):
        """transform -> (noise level per scale) -> thresholded inverse of x (B, n0), signal by signal, with ONE rows x n0 buffer.
        p (B, rows) float64: the thresholds, or (universal) the factor `scale` of lam = (scale sigma) sqrt(2 ln n0).  Returns
        (the sum with coeff = 1, sigma (B, rows) float64 -- not differentiable; zeros without `universal`).  Saved: x, the
        thresholds used (B, rows) and d lam / d scale -- not W."""
        @staticmethod
        def forward(ctx, x, p, eng, kind, param, dt, sj, mode, universal, columns, c, finite):
            nb, n0 = x.shape
            rows = sj.size
            out = torch.empty((nb, n0), dtype=x.dtype, device=x.device)
            sigma = torch.zeros((nb, rows), dtype=torch.float64, device=x.device)
            lam = torch.empty((nb, rows), dtype=x.dtype, device=x.device)
            tol = _tolerance()
            _begin(torch, eng, x.device, tol)
            W = torch.empty((rows, n0), dtype=_complex_of(torch, x.dtype), device=x.device)
            K = float(np.sqrt(2.0 * np.log(n0)))
            if universal:                                        # the ranks of the median over the columns [a, b), as row_quantiles
                a, b = columns
                lo = (b - a - 1) // 2
                ranks = [lo, lo + 1] if (b - a) % 2 == 0 else [lo]
                stats = torch.empty((rows, 8), dtype=x.dtype, device=x.device)
                first = a * (16 if x.dtype == torch.float64 else 8)
            for i in range(nb):
                if not finite[i]:                                # a non-finite sample: every element of W is NaN
                    out[i].fill_(float("nan"))
                    sigma[i].fill_(float("nan"))
                    lam[i].fill_(float("nan"))
                    continue
                eng.transform(x[i], n0, None, kind, param, dt, sj, W, n0)          # W as CwtRows.forward computes it
                if universal:
                    eng.plan.row_order_statistics(W.data_ptr() + first, True, n0, b - a, rows, ranks, stats.data_ptr(), 8)
                    # the roots, the mean of the two middle ones and the division as `noise_levels` does them, in NumPy on the
                    # host (rows x 2 numbers; one synchronisation per signal): the same bits as `denoise`, which a square root
                    # of torch's need not give
                    st = np.sqrt(stats[:, :len(ranks)].cpu().numpy().astype(np.float64))
                    med = 0.5 * (st[:, 0] + st[:, 1]) if len(ranks) == 2 else st[:, 0]
                    sigma[i] = torch.as_tensor(med / c, dtype=torch.float64).to(x.device)
                    lam[i] = ((p[i] * sigma[i]) * K).to(x.dtype)
                else:
                    lam[i] = p[i].to(x.dtype)
                shrink_inverse(eng, W, sj, lam[i], mode, out[i])
            del W
            ctx.save_for_backward(x, lam, sigma * K if universal else sigma)
            ctx.geometry = (eng, kind, param, dt, sj, tol, mode, universal, finite)
            ctx.mark_non_differentiable(sigma)
            return out, sigma

        @staticmethod
        @once_differentiable
        def backward(ctx, gy, _gsigma):
            x, lam, dlam = ctx.saved_tensors
            eng, kind, param, dt, sj, tol, mode, universal, finite = ctx.geometry
            nb, n0 = x.shape
            rows = sj.size
            g = gy.to(x.dtype).contiguous()
            xbar = torch.empty((nb, n0), dtype=x.dtype, device=x.device)
            glam = torch.empty((nb, rows), dtype=torch.float64, device=x.device)
            _begin(torch, eng, x.device, tol)
            G = torch.empty((rows, n0), dtype=_complex_of(torch, x.dtype), device=x.device)     # W recomputed, then its cotangent in place
            for i in range(nb):
                if not finite[i]:
                    xbar[i].fill_(float("nan"))
                    glam[i].fill_(float("nan"))
                    continue
                eng.transform(x[i], n0, None, kind, param, dt, sj, G, n0)
                eng.plan.icwt_shrink_adjoint(G.data_ptr(), n0, n0, sj, lam[i].data_ptr(), mode, 1.0, g[i].data_ptr(), G.data_ptr(), n0,
                                             glam[i].data_ptr())
                eng.adjoint_rows(G, n0, kind, param, dt, sj, xbar[i])
            del G
            return (xbar, glam * dlam if universal else glam) + (None,) * 10

    return SimpleNamespace(CwtRows=CwtRows, CwtPower=CwtPower, SsqRows=SsqRows, IcwtShrink=IcwtShrink, DenoiseRows=DenoiseRows)


def _learnable(name, torch, x, dj, s0, J, freqs, mother, scales, f0):
    """The checks of `scales=` and `f0=`: (the mother of this call, the scales as a float64 NumPy array or None)."""
    if f0 is not None:
        from .mothers import Morlet
        if type(mother) is not Morlet:
            raise ValueError(f"{name}: f0= is Morlet's parameter (Paul, DOG and duck-typed mothers have no differentiable one)")
        if not torch.is_tensor(f0) or f0.dim() != 0 or f0.dtype != torch.float64:
            raise ValueError(f"{name}: f0 must be a 0-dim float64 torch tensor")
        v = float(f0.detach())
        if not np.isfinite(v):
            raise ValueError(f"{name}: f0 must be finite")
        mother = Morlet(v)
    if scales is None:
        return mother, None
    if not (dj == 1 / 12 and s0 == -1 and J == -1 and freqs is None):
        raise ValueError(f"{name}: scales= replaces dj, s0, J and freqs; leave those at their defaults")
    if not torch.is_tensor(scales) or scales.dim() != 1 or scales.dtype != torch.float64 or scales.numel() < 1:
        raise ValueError(f"{name}: scales must be a 1-D float64 torch tensor")
    if scales.device.type != "cpu" and scales.device != x.device:
        raise ValueError(f"{name}: scales must live on the CPU or on x's device")
    sj = np.array(scales.detach().cpu().numpy(), dtype=np.float64)        # (a device tensor: one read-back per call)
    if not (np.isfinite(sj).all() and (sj > 0).all()):
        raise ValueError(f"{name}: scales must be positive and finite")
    return mother, sj


_Call = namedtuple("_Call", "torch eng kind param sj freqs coi hop keep")


def _prepare(name, x, dt, dj, s0, J, wavelet, freqs, pad, hop=None, scales=None, f0=None):
    """The checks, grid and engine of one call of `name` (cwt_torch, cwt_power_torch, ...).  `keep` is the mask of the scales
    that W keeps (Paul's NaN-row rule), for the way back of a gradient with respect to `scales`."""
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
    given = None
    if scales is not None or f0 is not None:
        mother, given = _learnable(name, torch, x, dj, s0, J, freqs, mother, scales, f0)
    if given is None:
        N, sj, freqs, coi, _, bad = _geometry(mother, n0, dt, dj, s0, J, freqs, True)
    else:                                                        # the grid is the caller's: no cache entry per step
        N, sj = _next_pow2(n0), given
        freqs, coi = 1 / (mother.flambda() * sj), _coi(mother, n0, dt)
        bad = _nan_rows(mother, sj, N, dt)
        bad = bad if bad.any() else None
    keep = np.ones(sj.size, dtype=bool)
    if bad is not None and not bad.all():
        sj, freqs, keep = sj[~bad], np.asarray(freqs)[~bad], ~bad
    sj, freqs, coi = np.array(sj, dtype=np.float64), np.array(freqs), np.array(coi)
    if hop is not None:
        hop = _check_hop(hop, N, mother)
        coi = coi[::hop]
    kind, param = _device_id(mother)
    nb = int(x.shape[0]) if x.dim() == 2 else 1
    precision = 64 if x.dtype == torch.float64 else 32
    eng = _engine(torch, N, precision, nb * sj.size, x.device, lib)
    return _Call(torch, eng, kind, float(param), sj, freqs, coi, hop, keep)


def cwt_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, pad=True, hop=None, *, scales=None, f0=None):
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
    choosing h against the smallest scale is the caller's business.

    scales=t (keyword only; a 1-D float64 torch tensor, positive and finite, on the CPU or on x's device) replaces the grid of
    ``dj, s0, J, freqs``, which must then stay at their defaults (ValueError otherwise), and makes W differentiable with
    respect to t.  f0=t0 (a 0-dim float64 tensor; Morlet only, ValueError for Paul, DOG or a duck-typed mother) replaces the
    wavelet object's f0 for this call and makes W differentiable with respect to it.  sj, freqs, coi come back as NumPy
    arrays of the detached values; scales that Paul's NaN-row rule drops from W get gradient 0.  The backward is ONE call of
    ``cwt_adjoint_rows_scales``: the adjoint with every row on its general path (the rows of polynomial form included) plus
    one reduction over each row's band, ``grad_scales = (dL/d ln s) / s``; x is saved and its spectrum recomputed there;
    x.grad is computed only if x requires it.  If neither tensor requires a gradient the backward is the one of the call
    without them.  Once differentiable.  A CPU tensor of scales is the cheap case: a tensor on the device costs one read-back
    (a host synchronisation) per call, because the grid is classified on the host.  A step with fresh scales re-classifies
    the grid there each time -- 1.9 ms for 256 scales at 2^20 points on the build machine (EXPERIMENTS.md); a whole step
    measured 8.2 ms against 6.0 with fixed scales (profiles/scale_grad_bench.txt) -- and a plan caches four row tables, so at
    most four distinct grids alternate for free."""
    call = _prepare("cwt_torch", x, dt, dj, s0, J, wavelet, freqs, pad, hop, scales, f0)
    W = _functions().CwtRows.apply(x.contiguous(), scales, f0, call.eng, call.kind, call.param, float(dt), call.sj, call.hop, call.keep)
    return W, call.sj, call.freqs, call.coi


def cwt_power_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, pad=True, hop=None, *, scales=None, f0=None,
                    pool=None):
    """The scalogram ``|W|^2`` of a torch tensor, differentiable with respect to it: ``cwt_torch(x, ...)[0].abs() ** 2`` without
    W -- neither written by the forward nor kept for the backward.

    Inputs, refusals, engine, stream and tolerance as ``cwt_torch``.  Returns ``(P, sj, freqs, coi)``: P float64 / float32 on
    x's device, (rows, n0) or (B, rows, n0), written by the power row kernels (``cwt_transform_power``).  Between forward and
    backward only x and the geometry of the call are held.  The backward recomputes W from x under the cotangent of P in the
    row kernels' store (``cwt_transform_weighted``: G = 2 gP W, complex, freed when the backward returns) and runs the HIP
    adjoint of the rows on G; once differentiable.

    hop=h as in ``cwt_torch``: P has ceil(n0 / h) columns, samples of |W|^2 at columns ``::h`` (not its mean over the hop), coi
    is ``coi[::h]``.  Forward, the transient G of the backward (``cwt_transform_hop`` with the weighted output) and its
    adjoint (``cwt_adjoint_rows_hop``) are all of rows x ceil(n0 / h) elements; x alone is saved.

    scales=, f0= (keyword only) as in ``cwt_torch``: P is differentiable with respect to them; the backward builds the same
    G = 2 gP W and hands it to ``cwt_adjoint_rows_scales``.

    pool=h (keyword only; a power of two, 2 <= h <= padded length; not together with hop): P has ceil(n0 / h) columns, the
    MEANS of |W|^2 over windows of h columns (the last window over its own columns), and coi is the minimum of coi over each
    window.  The forward is ``cwt_transform_pool``: the rows of polynomial form sum their windows in the kernel, nothing of
    rows x n0 elements is written for them, and x alone is saved.  The backward is NOT that small: the cotangent of W is
    G[j, n] = (2 / c_m) gP[j, n // h] W[j, n], built from what exists -- gP / c_m spread to n0 columns (Q, rows x n0 reals: 8 B
    per element in float64), ``cwt_transform_weighted`` with alpha = 2 (G, rows x n0 complex: 16 B per element), then
    ``cwt_adjoint_rows`` (with scales= / f0=: ``cwt_adjoint_rows_scales``) -- so it holds rows x n0 elements of Q and of G
    transiently, 24 B per element in float64, freed when it returns.  Once differentiable, like its siblings."""
    if pool is not None and hop is not None:
        _check_pool(pool, 2, hop=hop)
    call = _prepare("cwt_power_torch", x, dt, dj, s0, J, wavelet, freqs, pad, hop, scales, f0)
    coi = call.coi
    if pool is not None:
        pool, coi = _check_pool(pool, call.eng.plan.nfft), _pool_coi(coi, pool)
    P = _functions().CwtPower.apply(x.contiguous(), scales, f0, call.eng, call.kind, call.param, float(dt), call.sj, call.hop, call.keep,
                                    pool)
    return P, call.sj, call.freqs, coi


def ssq_cwt_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, *, gamma=None, ssq_freqs=None):
    """Synchrosqueezed wavelet transform of a torch tensor, differentiable with respect to it.

    x: (n0,) or (B, n0), float64 or float32, on a GPU (CPU tensors only under the CPU emulation of the library, as ``cwt_torch``).
    Returns ``(Tx, ssq_freqs, sj, freqs, coi)``: Tx complex, (nf, n0) or (B, nf, n0), on x's device and produced on torch's
    current stream, bin k at the ascending ``ssq_freqs[k]``; the grids are NumPy arrays as ``ssq_cwt`` returns them for the same
    call, the default ``ssq_freqs`` and the default gamma (``sqrt(eps) std(x)``, of every signal by itself) are those of
    ``ssq_cwt_device``.  Refusals as ``ssq_cwt``: DOG / MexicanHat and duck-typed mothers, ``freqs=`` without an explicit
    ``ssq_freqs=(f_lo, dv, nf)``; and nf > 32767 (the map of bins is int16).  A signal with a non-finite sample gives NaN in all of
    its Tx and NaN in its gradient.  Whether the signals are finite (and, by default, their standard deviations) is read back
    to the host: one synchronisation per call.

    Forward, signal by signal: W as ``cwt_torch`` computes it, dW from the spectrum times i w in row chunks
    (``cwt_transform_rows``), ``cwt_ssq_reassign_bins`` per chunk; W and dW are freed before it returns.  Given the bin of every
    entry T is linear in W, and the bins are piecewise constant in x: the gradient is exact almost everywhere and runs through
    the values of W alone.  Saved for the backward: the bins (int16, 2 B per entry of W) and the geometry -- not x, W or dW.
    Backward, signal by signal: ``cwt_ssq_gather`` of the cotangent through the bins into G (one signal's rows x n0), then
    ``cwt_adjoint_rows`` of G.  Once differentiable; no gradient with respect to the scales, gamma or the grid."""
    mother = _ssq_mother(wavelet)
    user_freqs = freqs is not None
    call = _prepare("ssq_cwt_torch", x, dt, dj, s0, J, mother, freqs, True)
    torch = call.torch
    f_lo, dv, nf = _ssq_grid(call.freqs, dj, ssq_freqs, user_freqs)
    if nf > 32767:
        raise ValueError("ssq_cwt_torch: at most 32767 bins (the map saved for the backward is int16)")
    xs = x.detach().reshape(-1, x.shape[-1])
    finite = torch.isfinite(xs).all(dim=1)
    if gamma is None:
        eps = float(np.finfo(np.float64 if x.dtype == torch.float64 else np.float32).eps)
        stat = torch.stack([finite.to(torch.float64), xs.to(torch.float64).std(dim=1, unbiased=False)]).cpu().numpy()
        gammas = [float(np.sqrt(eps) * s) if ok else None for ok, s in zip(stat[0], stat[1])]
    else:
        gamma = float(gamma)
        if not (np.isfinite(gamma) and gamma >= 0):
            raise ValueError("ssq_cwt: gamma must be finite and >= 0")
        gammas = [gamma if ok else None for ok in finite.cpu().numpy()]
    Tx = _functions().SsqRows.apply(x.contiguous(), call.eng, call.kind, call.param, float(dt), call.sj, (f_lo, dv, nf), gammas)
    return Tx, f_lo * 2.0 ** (dv * np.arange(nf)), call.sj, call.freqs, call.coi


def _icwt_coeff(mother, dt, dj):
    """dj sqrt(dt) / (cdelta psi(0)): a float where psi(0) is real, else complex"""
    coeff = complex(dj * np.sqrt(dt) / (mother.cdelta * mother.psi(0)))
    return coeff.real if coeff.imag == 0 else coeff


def issq_cwt_torch(Tx, dt, dj=1 / 12, wavelet="morlet", *, ssq_freqs=None, band=None):
    """Inverse of ``ssq_cwt_torch`` in plain torch operations (it differentiates by itself): ``dj sqrt(dt) / (cdelta psi(0))
    sum_k Re Tx[k, n]`` for Tx (nf, n0) or (B, nf, n0); band=(f1, f2) restricts the sum to the bins f1 <= ssq_freqs[k] < f2 (a
    component of the signal), the rule of ``issq_cwt``.  Real where the mother's psi(0) is."""
    import torch
    mother = _check_parameter_wavelet(wavelet)
    if not torch.is_tensor(Tx) or not Tx.is_complex() or Tx.dim() not in (2, 3):
        raise ValueError("issq_cwt_torch: Tx must be a complex tensor (bins x samples) or (B x bins x samples)")
    w = torch.as_tensor(_band_weights(ssq_freqs, Tx.shape[-2], band), dtype=Tx.real.dtype, device=Tx.device)
    total = (Tx.real * w[:, None]).sum(dim=-2)
    return total * _icwt_coeff(mother, dt, dj)


def _shrink_prepare(name, W, sj, wavelet):
    """The checks and the engine of `icwt_torch` / `icwt_shrink_torch`: (torch, engine, mother, sj, W as (B, rows, n0))."""
    import torch
    mother = _check_parameter_wavelet(wavelet)
    if not hasattr(mother, "device_id"):
        raise NotImplementedError(f"{name} needs a built-in mother (Morlet, Paul, DOG, MexicanHat); got {type(mother).__name__} "
                                  "without device_id()")
    if not torch.is_tensor(W) or W.dtype not in (torch.complex128, torch.complex64) or W.dim() not in (2, 3) or W.shape[-1] < 1:
        raise ValueError(f"{name}: W must be a complex torch tensor of shape (rows, n0) or (B, rows, n0)")
    sj = np.ascontiguousarray(sj, dtype=np.float64)
    if sj.shape != (W.shape[-2],) or not (np.isfinite(sj).all() and (sj > 0).all()):
        raise ValueError(f"{name}: sj must hold one positive scale per row of W")
    lib = _hip.load()
    if W.device.type != "cuda" and lib.backend().startswith("hip"):
        raise RuntimeError(f"{name} needs a tensor on a GPU (the HIP kernels cannot read host memory)")
    precision = 64 if W.dtype == torch.complex128 else 32
    eng = _engine(torch, _next_pow2(int(W.shape[-1])), precision, sj.size, W.device, lib)
    return torch, eng, mother, sj, (W if W.dim() == 3 else W[None]).contiguous()


def _check_mode(name, mode):
    if mode not in _wavelet.SHRINK_MODES:
        raise ValueError(f"{name}: mode must be one of {_wavelet.SHRINK_MODES}; got {mode!r}")
    return mode


def _rows_parameter(name, what, torch, t, nb, rows, batched, device):
    """`t` of shape (), (rows,) or (B, rows) -> a (B, rows) view of it on `device` (torch's expand: autograd sums)"""
    if not torch.is_tensor(t) or t.is_complex() or not t.is_floating_point():
        raise ValueError(f"{name}: {what} must be a real floating-point torch tensor")
    ok = t.dim() == 0 or tuple(t.shape) == (rows,) or (batched and tuple(t.shape) == (nb, rows))
    if not ok:
        raise ValueError(f"{name}: {what} must have shape (), ({rows},)" + (f" or ({nb}, {rows})" if batched else "")
                         + f"; got {tuple(t.shape)}")
    return t.to(device).expand(nb, rows)


def icwt_torch(W, sj, dt, dj=1 / 12, wavelet="morlet"):
    """Inverse wavelet transform of a torch tensor, differentiable with respect to it: ``icwt``'s series
    ``dj sqrt(dt) / (cdelta psi(0)) sum_j Re W[j, n] / sqrt(s_j)`` for W complex128 / complex64 of shape (rows, n0) or
    (B, rows, n0) on the device; (n0,) or (B, n0), real where the mother's psi(0) is.  The sum is ``cwt_icwt_reduce`` on torch's
    current stream, the factor a torch operation; the backward is ``cwt_icwt_shrink_adjoint`` without thresholds
    (G[j, n] = gy[n] / sqrt(s_j)): nothing is saved.  Built-in mothers; once differentiable."""
    torch, eng, mother, sj, Wb = _shrink_prepare("icwt_torch", W, sj, wavelet)
    total = _functions().IcwtShrink.apply(Wb, None, eng, sj, 0)
    return (total if W.dim() == 3 else total[0]) * _icwt_coeff(mother, dt, dj)


def icwt_shrink_torch(W, sj, dt, lam, dj=1 / 12, wavelet="morlet", mode="soft"):
    """``icwt_torch`` of the shrunk coefficients, differentiable with respect to W and to the thresholds: ``lam``, a real tensor
    of shape (), (rows,) or (B, rows), is the threshold on |W_j|; mode "hard" (keep |W| > lam), "soft" (W (1 - lam / |W|)+) or
    "garrote" (W (1 - lam^2 / |W|^2)+), the rules and roundings of ``cwt_icwt_shrink``.  The backward is
    ``cwt_icwt_shrink_adjoint``: the gradient of what the forward computed -- an entry on its threshold counts as dropped, the
    gradient with respect to lam is 0 in hard mode -- summed per row in one fixed order, in float64 across a row's slices.
    W and lam are saved (time-frequency masking between ``cwt_torch`` and here keeps W anyway); ``denoise_torch`` is the
    composition that does not.  Built-in mothers; once differentiable."""
    torch, eng, mother, sj, Wb = _shrink_prepare("icwt_shrink_torch", W, sj, wavelet)
    mode = _check_mode("icwt_shrink_torch", mode)
    lam_b = _rows_parameter("icwt_shrink_torch", "lam", torch, lam, Wb.shape[0], sj.size, W.dim() == 3, Wb.device)
    total = _functions().IcwtShrink.apply(Wb, lam_b.to(_real_of(torch, Wb.dtype)).contiguous(), eng, sj, mode)
    return (total if W.dim() == 3 else total[0]) * _icwt_coeff(mother, dt, dj)


def denoise_torch(x, dt, dj=1 / 12, s0=-1, J=-1, wavelet="morlet", freqs=None, *, mode="soft", threshold="universal", scale=1.0,
                  noise_columns=None):
    """Wavelet shrinkage of a torch tensor, differentiable with respect to it and to the thresholds: ``denoise`` as a layer.

    x: (n0,) or (B, n0), float64 or float32, on a GPU (CPU tensors only under the CPU emulation of the library, as
    ``cwt_torch``).  Returns ``(y, lam, sj, freqs, coi)``: y the denoised series on x's device, produced on torch's current
    stream, with the values of ``denoise`` for the same arguments (the same kernels in the same order); lam the thresholds used,
    a tensor (rows,) or (B, rows); sj, freqs, coi NumPy arrays as ``cwt`` returns them.

    threshold="universal": lam_j = scale sigma_j sqrt(2 ln n0), sigma_j the noise level of ``DeviceTransform.noise_levels``
    over ``noise_columns`` (all columns by default), selected on the device (``cwt_row_order_statistics``).  ``scale`` is a float
    or a tensor of shape () or (rows,) -- learnable: its gradient is that of lam times sigma_j sqrt(2 ln n0).  THE NOISE LEVELS
    ENTER AS CONSTANTS: the median is not differentiated, no gradient reaches x through sigma.  threshold=a tensor of shape (),
    (rows,) or (B, rows): the thresholds themselves, learnable (``scale`` does not apply, no selection runs).

    Between forward and backward the node holds x, the thresholds used (one per row and signal) and the geometry -- not W.  The
    backward, signal by signal: W recomputed into one rows x n0 buffer, overwritten in place by its cotangent
    (``cwt_icwt_shrink_adjoint``, which also sums the cotangent of the thresholds), ``cwt_adjoint_rows``, the buffer freed.  A
    signal with a non-finite sample gives NaN in its y and in its gradients (one read-back of the flags per call).  Built-in
    mothers, pad=True, no hop; the refusals of ``denoise``; once differentiable."""
    mode = _check_mode("denoise_torch", mode)
    if isinstance(threshold, str) and threshold != "universal":
        raise ValueError(f'denoise_torch: threshold must be "universal" or a tensor of thresholds; got {threshold!r}')
    mother = _check_parameter_wavelet(wavelet)
    if not hasattr(mother, "device_id"):
        raise NotImplementedError("denoise_torch needs a built-in mother (Morlet, Paul, DOG, MexicanHat from pycwt_amd); "
                                  f"got {type(mother).__name__} without device_id()")
    call = _prepare("denoise_torch", x, dt, dj, s0, J, mother, freqs, True)
    torch, sj = call.torch, call.sj
    from .mothers import DOG
    nb, n0, rows = (int(x.shape[0]) if x.dim() == 2 else 1), int(x.shape[-1]), sj.size
    universal = isinstance(threshold, str)
    columns = (0, n0)
    if universal:
        if noise_columns is not None:
            columns = (int(noise_columns[0]), int(noise_columns[1]))
            if not 0 <= columns[0] < columns[1] <= n0:
                raise ValueError(f"columns must be (a, b) with 0 <= a < b <= {n0}; got {noise_columns!r}")
        if not torch.is_tensor(scale):
            scale = torch.tensor(float(scale), dtype=torch.float64)
        if scale.dim() == 2:
            raise ValueError("denoise_torch: scale must be a float or a tensor of shape () or (rows,)")
        p = _rows_parameter("denoise_torch", "scale", torch, scale, nb, rows, False, x.device)
    else:
        p = _rows_parameter("denoise_torch", "threshold", torch, threshold, nb, rows, x.dim() == 2, x.device)
    xs = x.reshape(nb, n0).contiguous()
    finite = [bool(v) for v in torch.isfinite(xs.detach()).all(dim=1).cpu().numpy()]
    c = 0.6744897501960817 if isinstance(mother, DOG) else float(np.sqrt(np.log(4.0)))
    total, sigma = _functions().DenoiseRows.apply(xs, p.to(torch.float64), call.eng, call.kind, call.param, float(dt), sj, mode, universal,
                                                  columns, c, finite)
    lam = (p.to(torch.float64) * sigma) * float(np.sqrt(2.0 * np.log(n0))) if universal else p
    y = total * _icwt_coeff(mother, dt, dj)
    if x.dim() == 1:
        y, lam = y[0], lam[0]
    return y, lam, sj, call.freqs, call.coi


def _ssq_saved_bins(Tx):
    """The map a ``Tx`` of ``ssq_cwt_torch`` holds for its backward (tests): int16, (..., rows, n0), the bin of every kept entry
    of W and -1 of every dropped one.  Only a Tx that requires a gradient holds one."""
    fn = getattr(Tx, "grad_fn", None)
    if fn is None or not getattr(fn, "ssq_map", False):
        raise ValueError("not the output of ssq_cwt_torch for an input that requires a gradient")
    return fn.saved_tensors[0]
