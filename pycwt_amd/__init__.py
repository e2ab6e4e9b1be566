"""pycwt_amd -- MI355X-native engine for pycwt's FFT-convolution CWT hot path.

``cwt`` / ``icwt`` keep the signatures of regeirk/pycwt (pycwt/__init__.py:85-90 re-exports them
from pycwt/wavelet.py); the arithmetic runs in hand-written HIP kernels (pycwt_amd/csrc) reached
through the C ABI of include/cwt_hip.h.  Importing this package does not need a GPU; calling
``cwt`` / ``icwt`` does, and fails loudly without one.
"""
from . import helpers, mothers
from .helpers import ar1, ar1_spectrum, fft, fft_kwargs, find, get_cache_dir, rednoise
from .mothers import DOG, MexicanHat, Morlet, Paul
from .wavelet import (DeviceCoherence, DevicePower, DeviceTransform, cwt, cwt_batch, cwt_device, cwt_power, cwt_power_batch,
                      cwt_power_device, denoise, icwt, release_scratch, set_tolerance, DeviceSynchrosqueezed, issq_cwt, ssq_cwt, ssq_cwt_device,
                      significance, wct, wct_device, wct_significance, xwt, xwt_device)

from .autograd import cwt_power_torch, cwt_torch, denoise_torch, icwt_shrink_torch, icwt_torch, issq_cwt_torch, ssq_cwt_torch

__version__ = "0.1.0"
__all__ = ["cwt", "cwt_torch", "cwt_power_torch", "ssq_cwt_torch", "issq_cwt_torch", "icwt_torch", "icwt_shrink_torch", "denoise_torch", "cwt_batch", "cwt_device", "DeviceTransform", "cwt_power", "cwt_power_batch", "cwt_power_device",
           "DevicePower", "DeviceCoherence", "ssq_cwt", "ssq_cwt_device", "issq_cwt", "DeviceSynchrosqueezed", "wct_device", "xwt_device", "icwt", "denoise", "set_tolerance", "release_scratch", "significance", "xwt", "wct", "wct_significance", "Morlet", "Paul", "DOG",
           "MexicanHat", "ar1", "ar1_spectrum", "rednoise", "find", "get_cache_dir", "helpers", "mothers", "fft", "fft_kwargs"]
