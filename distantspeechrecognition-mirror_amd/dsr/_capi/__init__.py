"""ctypes binding of libdsr_hip.so (include/dsr.h).

This is plumbing: device memory and streams come from torch (ROCm), every compute call goes
through the C-ABI with raw device pointers.  There is no CPU path here; if the shared library or
a HIP device is missing the call raises.

One module per reference module, under the names dsr/btk and dsr/asr use (the rule of csrc/stream_op.h); _core holds what they share.
This file only re-exports: `import dsr._capi as K` and `from dsr._capi import X` see every name of every module.
"""
# flake8: noqa: F401
from . import _core
from ._core import (C, os, re, np, _HERE, _LIBPATH, _HEADER, _SCALARS, _ctype_of, header_prototypes, declare_from_header, load, check, cur_stream,
                    DsrError, ERROR_NAMES, E_ITERATOR, E_IO, E_INDEX, E_DIMENSION, E_CONSISTENCY, E_KEY, E_PARAMETER, E_PARSE, MfccCfg, DecoderCfg,
                    DecodeResult, vp, i32, i64, f32, f64, u32, _np, _ptr, _dev, _nf, _state, _batch)
from .modulated import (FilterBank, FilterBankState, PrFilterBank, NormalFFTBank)
from .beamformer import (Beamformer, calcDelaysPolar2, RLS_STATE_REGS, RLS_STATE_LDS, RLS_STATE_MEM, bf_rls_path, SubbandMMI, DoaSRP, _Sph,
                         SphBeamformer, SphDoaSRP, sph_beams_cell, SphTracker, PlaneWaveSim, MK_PR, MK_NRM, MK_EXIT_MAX_ITERATIONS, MK_EXIT_GRADIENT,
                         MK_EXIT_DIFFERENCE, MK_EXIT_NO_PROGRESS, MK_EXIT_EVAL_CAP, MK_EXIT_SKIPPED, MK_FRAMES_LDS, MK_FRAMES_STREAMED, MK_EVAL_CAP,
                         mk_path, MkBeamformer)
from .localization import (Gcc, cctde, SearchGrid, mcc_check, MccLocalizer, MccCalculator)
from .enhance import (wpe_single, wpe_multi, Aec)
from .postfilter import (PF_ZEL_REG, PF_ZEL_SUM, PF_ZEL_SUM_BF, PF_MCCOWAN_REG, PF_MCCOWAN_MEM, PF_WAVE, zelinski_path, ZelinskiPostFilter,
                         McCowanPostFilter, LefkimmiatisPostFilter, SpectralSubtractor, WienerFilter, BinaryMask, ThresholdEstimator, psdFileWrite,
                         psdFileRead)
from .feature import (LpcEnvelope, WtMvdrEnvelope, spectral_smoothing, BlockConvolver, fir_frames, fir_frames_count, signal_power, zero_crossing_rate,
                      yin_pitch, yin_kernel, spike_filter, spike_filter2_state, spike_filter2, minmax_state, alog, normalize, threshold, amplify,
                      SPECTRAL_SAMPLE_RATIO, spectral_resample, SphinxMel, MFCC_FRAMES_PLAIN, MFCC_FRAMES_W, MFCC_CMN_NONE, MFCC_CMN_PLAIN,
                      MFCC_CMN_LDS, MFCC_LDA_TOO_LARGE, MFCC_LDA_SPLICE, MFCC_LDA_PLAIN, MFCC_LDA_B, mfcc_cfg_paths, Mfcc)
from .sad import (_sad_out, sad_energy_state, sad_energy_reset, sad_energy, sad_energy_percentile, sad_simple_energy, sad_band, SAD_POWER_RATIO,
                  SAD_ENERGY_RATIO, SAD_TSPS, sad_power, sad_ccc, SAD_HANGOVER, SAD_HANGOVER_MI, SAD_HANGOVER_MULTISTAGE, sad_hangover, sad_gather,
                  SAD_ENERGY_DIFFUSION, SAD_BAND_ENERGY_RATIO, SAD_NEGATIVE_ENTROPY, SAD_SIGNIFICANT_SUBBANDS, sad_shape, SAD_NEGENTROPY,
                  SAD_MUTUAL_INFORMATION, SAD_LIKELIHOOD_RATIO, sad_read_shape_factors, SadGG)
from .gaussian import (Gmm, Trainer)
from .adapt import (is_ancestor, ParamTree, Mllr, Fsa, _Estimators, Stc, Lda)
from .decoder import (Wfst, Decoder, _lexh, Lattice, Pipe)
_LAZY = dict(AdaptiveBeamformer="_abf", SampleRateConverter="_src", AptParams="_apt", Apt="_apt", apt_line_search="_apt", apt_transform_rows="_apt", APT_BIAS="_apt", APT_RAPT="_apt", APT_SLAPT="_apt", Sat="_sat", speaker_list_read="_sat", sat_check="_sat", SAT_MEAN="_sat", SAT_VARIANCE="_sat", SAT_MLLR="_sat", SAT_APT="_sat", FastSat="_fsat", fsat_check="_fsat")

def __getattr__(name):
    if name == "_lib":                                 # the loaded library, live: _core owns it, load() rebinds it
        return _core._lib
    if name in _LAZY:                                  # include/dsr.h sections 2a'', 6d, 13, 14, 14b: dsr/_abf.py, _src.py, _apt.py, _sat.py, _fsat.py, on the common handle base
        import importlib; return getattr(importlib.import_module(".." + _LAZY[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
