"""opticomlib_amd -- the split-step Fourier fibre path of opticomlib on AMD Instinct MI355X.

Drop-in for ``opticomlib.devices.FIBER`` / ``DBP`` / ``DM``, the zero-phase filters ``LPF`` / ``BPF`` and
the receiver front-end ``PD`` / ``EDFA``, the fibre Bragg grating ``FBG``, the phase modulator ``PM``, the quantiser ``ADC``, the OOK receiver ``GET_EYE`` / ``SAMPLER`` / ``ook``, the PPM receiver ``ppm``, the data-aided receiver ``lab.SYNC`` / ``lab.GET_EYE_v2``, the coherent QAM receiver ``coherent``, the eye's ``plot``, Welch's spectrum ``get_psd`` and the signals' ``.psd()`` plots (and the slice of ``optical_signal`` / ``electrical_signal`` /
``gv`` they touch); everything else of opticomlib is out of scope.
The arithmetic runs in hand-written HIP kernels (``csrc/``) behind the C ABI declared in
``include/ssfm_amd.h``.
"""
from .typing import NULL, EyeShowOptions, binary_sequence, electrical_signal, eye, gv, optical_signal
from .devices import ADC, BPF, DAC, DBP, DM, EDFA, FBG, FIBER, GET_EYE, LASER, LPF, MZM, PD, PM, PRBS, SAMPLER, device_rng_seed
from . import coherent, lab, ook, ppm
from .utils import eye_density, eye_fold_density, eyediagram, get_psd
from ._lib import C64, C128, Plan, SsfmError, device_count

__all__ = ["NULL", "gv", "optical_signal", "electrical_signal", "FIBER", "DBP", "DM", "LPF", "BPF", "PD", "EDFA", "PRBS", "DAC", "LASER", "MZM", "PM", "FBG", "ADC", "GET_EYE", "SAMPLER", "ook", "ppm", "lab", "coherent", "get_psd", "eye_density", "eyediagram", "eye_fold_density", "eye", "EyeShowOptions", "binary_sequence", "device_rng_seed", "Plan", "SsfmError", "device_count", "C64", "C128"]
__version__ = "0.1.0"
